// kernels.h -- host-side launchers of every HIP kernel in libsamrs_hip (internal header).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- gemm.hip (the dispatch) and the kernel families beside it: gemm_ring / gemm_dual / gemm_decoder / gemm_experiments.hip ------
// Which kernel runs a launch is decided by gemm_select (gemm_select.h) from the shape, the flags and the variant in force.
struct GemmOpts {
    int ld = 0;           // row stride of A and B in elements (>= K, a multiple of 8), 0 = K: the persistent ET kernels alone read with it (gemm_ld_ok says whether
                          // a launch of the shape runs on one of them; anything else refuses a stride)
    int gelu_form = 1;    // erf form of their GELU epilogue (lin1): 1 = fp32-epsilon class, 2 = cheaper
};
hipError_t launch_gemm_et(int prec, const void* A, const void* B, void* C, const float* bias,
                          const float* add2d, int add2d_period, int M, int N, int K, bool out_f32,
                          bool gelu, bool accumulate, hipStream_t s, GemmOpts opts = {});
// the rule's answer for such a call under `variant`, nothing launched: out8 = kernel (enum GemmKernel), ni, mode, persistent, reject,
// gemm_ld_ok(M, N, K, gelu), gemm_ext_ok(M, N, K), gemm_lntail_ok(M, N, K) as they answer under that variant
void gemm_debug_choice(int prec, int M, int N, int K, bool out_f32, bool gelu, bool accumulate, bool has_add2d, int ld, int variant,
                       int32_t* out8);
// C (ET) = GELU(LayerNorm2d over every 64-column group of (A B^T + bias)), eps 1e-6; gamma_beta = gamma[64] | beta[64]
// A_lo / B_lo (both or neither): split-precision product of hi + lo operands; C is then FP32 [M][N] instead of ET
hipError_t launch_gemm_et_gln(int prec, const void* A, const void* B, void* C, const float* bias, const float* gamma_beta,
                              int M, int N, int K, hipStream_t s, const void* A_lo = nullptr, const void* B_lo = nullptr);
// LayerNorm folded into the neighbouring GEMMs (residual stream of N = 1280 columns):
//   producer  C (fp32) += A B^T + bias;  Xh = ET(C);  stats[m][N / 160] = (mean, sum of squared deviations) per 160 columns
//   (launch_ln_rowstat, encoder_kernels.hip: stats -> rowstat[m] = (rstd, -rstd mean))
//   consumer  C (ET) = [GELU](rstd_m (Xh Wf^T - mean_m cvec) + bias_f)
hipError_t launch_gemm_et_stats(int prec, const void* A, const void* B, float* C, const float* bias, void* Xh, float* stats,
                                int M, int N, int K, hipStream_t s);
hipError_t launch_gemm_et_fold(int prec, const void* Xh, const void* Wf, void* C, const float* bias_f, const float* cvec,
                               const float* rowstat, int M, int N, int K, bool gelu, hipStream_t s);
// Split-precision product in ONE launch: C = A B^T + A_lo B^T + A B_lo^T + bias over a three-segment K axis (fp32 accumulators stay
// in registers).  out_f32: C is fp32 [M][N] (optionally accumulated into), else ET rounded once.  gemm_split3_ok: M % 256,
// N % 320, K % 64 (the ViT-H block GEMMs); other shapes take three accumulating launch_gemm_et passes.
bool gemm_split3_ok(int M, int N, int K, bool out_f32 = false);      // fp32 outputs also take N % 256 == 0 (the neck)
hipError_t launch_gemm_et_split3(int prec, const void* A, const void* A_lo, const void* B, const void* B_lo, void* C, const float* bias,
                                 int M, int N, int K, bool out_f32, bool accumulate, hipStream_t s, int split_from_n = 0,
                                 const float* add2d = nullptr, int add2d_period = 0);   // add2d: fp32 outputs only (patch embed + pos_embed)
// split_from_n (ET output only, a multiple of 320): only output columns >= split_from_n take the lo terms; the tiles in front
// of it are the plain hi x hi product (qkv: the v third alone)
void set_gemm_variant(int v);   // process-wide test hook (kernel-level entry points): 0 = register-staged tiles, ..., 8 = automatic
// proj / lin2 with the LayerNorm that follows them as a tail of the GEMM (gemm.hip gemm_et_x64_kernel<LNT>): C (fp32) += A B^T + bias,
// out_et = LN(C) in the operand type; hipErrorInvalidValue where the shape does not take that kernel (caller: separate launches)
bool gemm_has_experiments();     // built with -DSAMRS_EXPERIMENTS (make EXPERIMENTS=1): the 32x32x16 GEMM kernels, the LayerNorm fold, the timing ablations
bool gemm_lntail_ok(int M, int N, int K);
hipError_t launch_gemm_et_lntail(int prec, const void* A, const void* B, float* C, const float* bias, int M, int N, int K,
                                 const float* gamma, const float* beta, float eps, void* out_et, unsigned int* counters, hipStream_t s);
bool gemm_ld_ok(int M, int N, int K, bool gelu);     // a plain ET launch of this shape takes an operand row stride (GemmOpts::ld)
// C (fp32 [M][N], the residual stream) += A B^T + A_x B_x^T + bias: proj / lin2 with ONE more 64-k stage read from two dense side operands
// A_x [M][64], B_x [N][64] (hi + lo of the outlier columns, engine_state.h EncBlock::oc_*).  gemm_ext_ok: the shapes of the 256 x 320
// pair-stage kernel (ViT-H at >= 2 tiles); other shapes add the side product with an accumulating launch of their own.
bool gemm_ext_ok(int M, int N, int K);
hipError_t launch_gemm_et_ext(int prec, const void* A, const void* B, const void* Ax, const void* Bx, float* C, const float* bias,
                              int M, int N, int K, hipStream_t s);
int swap_gemm_variant_override(int v);   // thread-local override (-1 = none) used by engine handles; returns the previous value
void set_gemm_skew(int xcd_units, int cu_units);   // first-round start skew of the pair-stage GEMM (1024-cycle units)
hipError_t launch_gemm_f32(const float* A, int lda, const float* W, const float* bias, float* C,
                           int ldc, int M, int N, int K, bool relu, bool accumulate, hipStream_t s);
// up to F32_BATCH_MAX same-shape fp32 GEMMs in one launch: C[z] = (A[z] (+ A2[z])) * W[z]^T + bias[z]
constexpr int F32_BATCH_MAX = 5;
struct F32Batch {
    const float* A[F32_BATCH_MAX];
    const float* A2[F32_BATCH_MAX];     // optional elementwise addend of A (same lda), or null
    const float* W[F32_BATCH_MAX];
    const float* bias[F32_BATCH_MAX];   // or null
    float* C[F32_BATCH_MAX];
};
hipError_t launch_gemm_f32_batch(const F32Batch& bt, int count, int lda, int ldc, int M, int N, int K, bool relu,
                                 bool accumulate, hipStream_t s);

// ---- encoder_kernels.hip --------------------------------------------------------------------
// A_lo / out_lo (optional): the remainder of the two-term operand split (common.h split2_pack), same layout as the main output
hipError_t launch_patch_im2col(int prec, const uint8_t* img, void* A, int n_images, int in_h, int in_w,
                               int grid, int patch, hipStream_t s, void* A_lo = nullptr);
hipError_t launch_convert(int prec, const float* in, void* out, long n, hipStream_t s, void* out_lo = nullptr);
// folded LayerNorm (ViT-H): weight preparation (once) and the entry of the folded path (Xh = ET(X) + per-row partial statistics)
hipError_t launch_ln_fold_weight(int prec, const float* W, const float* gamma, const float* beta, const float* bias, void* Wf,
                                 float* cvec, float* bias_f, int N, int K, hipStream_t s);
hipError_t launch_rowstats_convert(int prec, const float* X, void* Xh, float* stats, int rows, int D, hipStream_t s);
// stats [rows][8] (mean, M2) of 160-element groups -> rowstat [rows] = (rstd, -rstd mean), Chan merge in a fixed order
hipError_t launch_ln_rowstat(const float* stats, float* rowstat, int rows, float eps, hipStream_t s);
hipError_t launch_layernorm(int prec, const float* X, const float* gamma, const float* beta, float eps,
                            void* out_et, float* out_f32, int rows_out, int D, int window_mode, int grid,
                            int window, hipStream_t s, void* out_lo = nullptr,
                            // optional (plain row order, D % 256 == 0): the output's hi / lo as MXFP4 codes [rows][D / 2] + scale tiles
                            // (the A operands of launch_gemm_et_mx: no ET lo copy, no separate pack pass)
                            void* mx_q_hi = nullptr, void* mx_q_lo = nullptr, void* mx_s_hi = nullptr, void* mx_s_lo = nullptr,
                            int ld_out = 0 /* row stride of out_et in elements, 0 = D (plain ET output only) */,
                            // optional (plain row order, ld_out >= D + 64): hi + lo of n_oc <= 32 outlier columns as 64 more K columns
                            // of the row: [D + j] = lo of column oc_idx[j], [D + 32 + j] = its hi, zeros in unused slots
                            const int* oc_idx = nullptr, int n_oc = 0);
// weight side of that extension: out[r][col0 + j] = ET(W[r][idx[j]]), out[r][col0 + 32 + j] = ET(W - hi), W fp32 [N][K], out rows of stride ld
hipError_t launch_outlier_weight_ext(int prec, const float* W, int N, int K, const int* idx, int n_oc, void* out, int ld, int col0, hipStream_t s);
// the producers of the side operands of proj / lin2 (launch_gemm_et_ext): see the kernels in encoder_kernels.hip
hipError_t launch_outlier_side_weight(int prec, const float* W1, const float* b1, int D, const int* idx2, int n2, const int* idx1, int n1,
                                      void* out, int Ks, float* bias_out, hipStream_t s);
hipError_t launch_outlier_gather(const void* hi, const void* lo, int D, const int* idx, int n_oc, void* out, int rows, hipStream_t s);
// lin2's A_x: out [M][64] = lo | hi of GELU(Y Ws^T + bias), Y [M][K] with row stride lda, Ws [32][K], bias [32]; M % 64 == 0, K % 32 == 0
hipError_t launch_outlier_side_gemm(int prec, const void* Y, int lda, const void* Ws, const float* bias, int M, int K, void* out, hipStream_t s);
// squared L2 norms of the columns / rows of an fp32 matrix [N][K] (either output may be null); load-time scoring of outlier columns
hipError_t launch_weight_norms(const float* W, int N, int K, float* col_sq, float* row_sq, hipStream_t s);
// out_lo (optional, both attention kernels): the split remainder of `out` (reference-grade mode: proj on hi + lo operands)
hipError_t launch_window_attention(int prec, const void* qkv, const float* qkv_bias, const float* rel_h, const float* rel_w, void* out,
                                   int n_images, int grid, int window, int heads, int head_dim, hipStream_t s, void* out_lo = nullptr,
                                   // optional (instead of out_lo): hi / lo of the output as MXFP4 on the per-head padded K axis
                                   // [rows][heads * ceil32(head_dim) / 2], block-internal order of store_attention_row_mx
                                   void* mx_q_hi = nullptr, void* mx_q_lo = nullptr, void* mx_s_hi = nullptr, void* mx_s_lo = nullptr,
                                   // out_lo only: bit h set = head h writes its remainder (default: every head)
                                   uint32_t lo_heads = 0xffffffffu);
hipError_t launch_gelu_split(int prec, const float* in, void* hi, void* lo, long n, hipStream_t s);
// operand-range check: adds to *counter the elements of an ET tensor that sit at the operand type's saturation value or beyond (n % 8 == 0)
hipError_t launch_range_scan(int prec, const void* x, long n, unsigned long long* counter, hipStream_t s,
                             int cols = 0, int ld = 0 /* optional: rows of `cols` live elements at a stride of `ld` elements; n = rows * cols */);
// vt_ws: ET workspace of n_images * heads * head_dim * grid^2 elements (receives V transposed per head)
hipError_t launch_global_attention(int prec, const void* qkv, const float* rel_h, const float* rel_w, void* out,
                                   int n_images, int grid, int heads, int head_dim, void* vt_ws, hipStream_t s, void* out_lo = nullptr,
                                   void* mx_q_hi = nullptr, void* mx_q_lo = nullptr, void* mx_s_hi = nullptr, void* mx_s_lo = nullptr);
hipError_t launch_neck_im2col(const void* in, void* A, int n_images, int grid, int C, hipStream_t s);
hipError_t launch_transpose_f32(const float* in, float* out, int rows, int cols, hipStream_t s);

// ---- audit_kernels.hip (engine options "range_profile" / "audit_passes") ---------------------
constexpr int AUDIT_PROFILE_WORDS = 48;        // int64 words of one profile row (layout: samrs_hip.h samrs_audit_read_profile)
constexpr int AUDIT_ROWS_PER_PARTIAL = 256;    // rows one fp32 partial of the column statistics sums in sequence
// adds the profile of an ET tensor (n elements as rows of `cols` live elements at a stride of `ld`; cols <= 0: dense; all % 8 == 0)
// into row48: integer atomics only, the result does not depend on the order of the blocks
hipError_t launch_range_profile(int prec, const void* x, long n, int cols, int ld, long long* row48, hipStream_t s);
// per column of an ET matrix [M][K] (row stride ld): sumsq[c] += sum of squares (fp32 chains of AUDIT_ROWS_PER_PARTIAL rows stored to
// partials [column_stats_partial_floats(M, K)], added in slab order in fp64), maxbits[c] = max(maxbits[c], bits & 0x7fff)
size_t column_stats_partial_floats(int M, int K);
hipError_t launch_column_stats(int prec, const void* x, int M, int K, int ld, float* partials, double* sumsq, uint32_t* maxbits, hipStream_t s);

// ---- decoder_kernels.hip --------------------------------------------------------------------
struct PromptParams {
    const float* boxes;          // [n,4] or null
    const float* point_coords;   // [n,np,2] or null
    const int32_t* point_labels; // [n,np] or null
    int n_prompts, n_points;
    float img_size;
    const float* gauss;          // [2,128]
    const float* point_emb[4];   // 4 x [256]
    const float* not_a_point;    // [256]
    const float* iou_token;      // [256]
    const float* mask_tokens;    // [4,256]
};
// tokens [n, T, 256], T = 5 + n_points (+1 pad point when there is no box) + 2*(boxes != null)
hipError_t launch_prompt_tokens(const PromptParams& p, float* tokens, float* tokens2 /* optional second copy */, int T, hipStream_t s);
hipError_t launch_dense_pe(const float* gauss, float* pe /*[g*g,256]*/, int grid, hipStream_t s);
// mask prompt -> dense embedding [n, 4096, 256] (prompt_encoder.py:51-59)
struct MaskEmbedParams {
    const float *w0, *b0, *ln1w, *ln1b, *w3, *b3, *ln4w, *ln4b, *w6, *b6;
};
hipError_t launch_mask_embed(const MaskEmbedParams& p, const float* mask_in, float* dense, int n, int grid, hipStream_t s);
// out_f32[b, t, :] = emb[t, :] + (dense ? dense[b, t, :] : vec[:]) and its ET copy
// (slot_of: emb[slot_of[b], t, :] instead, emb then being the [slots][tokens][C] embedding store)
// per-prompt slot table on the stream: out[p] = slot[k] for p in [start[k], start[k + 1]), k < n_runs (host arrays,
// passed by value in the kernel arguments, so nothing reads them after the call returns)
hipError_t launch_fill_slot_table(const int* start, const int* slot, int n_runs, int* out, hipStream_t s);
hipError_t launch_make_keys(int prec, const float* emb, const float* dense, const float* vec, float* out_f32,
                            void* out_et, int n_batches, int tokens, int C, hipStream_t s, const int* slot_of = nullptr);
hipError_t launch_add_f32(const float* a, const float* b, float* out, long n, hipStream_t s);
// token self attention: q,k,v [n*T, C] -> o [n*T, C]; heads of dim C/heads
hipError_t launch_token_self_attn(const float* q, const float* k, const float* v, float* o, int n, int T, int C,
                                  int heads, hipStream_t s);
// tokens -> image attention. qp [n*T, Ci] fp32; kp/vp ET rows of `ld` elements, batch stride in rows
// (0 = shared by all prompts); o [n*T, Ci] fp32.  slot_of (device int [n], optional): prompt b reads the rows of batch
// slot_of[b] instead of batch b -- the layer-0 keys of several images' slots in one launch (samrs_predict_multi).
constexpr int T2I_MAX_SPLITS = 16;
size_t t2i_workspace_floats(int n_prompts, int T);     // scratch for the per-split partial softmax states
hipError_t launch_t2i_attention(int prec, const float* qp, const void* kp, const void* vp, int ld, long batch_stride_rows,
                                float* out, float* workspace, int n, int T, int tokens, int Ci, int heads, hipStream_t s,
                                const int* slot_of = nullptr);
// image -> tokens attention. qi ET rows of `ld` elements (batch stride in rows, 0 = shared);
// kt, vt [n*T, Ci] fp32; out ET [n*tokens, Ci].
hipError_t launch_i2t_attention(int prec, const void* qi, int ld, long batch_stride_rows, const float* kt,
                                const float* vt, void* out, int n, int T, int tokens, int Ci, int heads, hipStream_t s);
// per row of `in` [rows, groups*gsize]: +0, LN over each group (eps), GELU -> ET
hipError_t launch_group_ln_gelu(int prec, const float* in, const float* gamma, const float* beta, float eps,
                                void* out, long rows, int groups, int gsize, hipStream_t s);
// low[b, c, Y, X] = sum_ch hyper[b, sel0 + c, ch] * up2[b, y, x, dy, dx, dy2, dx2, ch]
// fused ConvT #2 (K = 64 GEMM) + GELU + hypernetwork product: u1 [n*grid*grid*4][64] ET -> low [n][n_sel][4 grid][4 grid]
// w_lo != null: split precision -- u1 is then the FP32 output of the first transposed conv [rows][64] (split in registers)
hipError_t launch_upscale2_masks(int prec, const void* u1, const void* w, const void* w_lo, const float* bias, const float* hyper,
                                 float* low, int n, int grid, int n_mask_tokens, int sel0, int n_sel, hipStream_t s);
hipError_t launch_mask_product(int prec, const void* up2, const float* hyper, float* low, int n, int grid,
                               int n_mask_tokens, int sel0, int n_sel, hipStream_t s);
hipError_t launch_postprocess(const float* low, int n_masks, int in_h, int in_w, int orig_h, int orig_w,
                              int img_size, int return_logits, void* out, hipStream_t s);
hipError_t launch_paint(const uint8_t* masks, const int32_t* labels, int n, int h, int w, uint8_t* seg,
                        unsigned long long* areas, unsigned long long* class_pixels,
                        unsigned long long* class_instances, int n_classes, hipStream_t s);
// best-of-nsel by predicted IoU (first maximum): out [n][h][w] = masks[j][argmax_c iou[j][c]], quality[j], areas[j] = pixels set
hipError_t launch_select_best(const uint8_t* masks, const float* iou, int n, int nsel, int h, int w, uint8_t* out, float* quality,
                              unsigned long long* areas, hipStream_t s);
// ground-truth matching: inter[j] = |mask j AND (label == colors[j])|, gt_area[j] = |label == colors[j]|; gt_masks [n][h][w] 0/1 or null
hipError_t launch_gt_match(const uint8_t* masks, int n, int h, int w, const uint8_t* label_rgb, const uint8_t* colors,
                           unsigned long long* inter, unsigned long long* gt_area, uint8_t* gt_masks, hipStream_t s);
hipError_t launch_resample_pass(const uint8_t* in, uint8_t* out, const int32_t* bounds, const int32_t* coef, int ksize,
                                int in_len, int out_len, int other, int horizontal, hipStream_t s);
// rotated-box polygons (int32 [n][nv][2]) -> mask prompts [n][out][out] fp32 (main_sam_rbox_mask_instance.py:125-141)
hipError_t launch_rbox_prompt(const int32_t* pts, int n, int nv, int h, int w, int th, int tw, int img_size, int out_size,
                              float* out, hipStream_t s,
                              int fill_rule = 0 /* 0: OpenCV <= 4.5.1 spans (ceil .. floor), 1: OpenCV >= 4.5.2 (round .. round) */);
// fused transformer.py:176-181: keys = LayerNorm(resid + out_proj(attention(q_i2t, k_tokens, v_tokens))) -> outF (fp32) and outE (ET)
// slot_of: as in launch_t2i_attention, for the query side and the residual (q_bstride / r_bstride then stride slots)
hipError_t launch_i2t_fused(int prec, const void* qi, int ld, long q_bstride, const float* kt, const float* vt, const void* w,
                            const void* w_lo /* null: un-split out-projection */, const float* bias, const float* resid,
                            long r_bstride, const float* gamma, const float* beta, float eps, float* outF, void* outE,
                            void* outE_lo /* optional split remainder of outE */, int n, int T, int tokens, int Ci, int C, hipStream_t s,
                            const int* slot_of = nullptr);

// ---- gemm.hip: operand split with the two correction terms on MXFP4 operands (gemm_et_mx_kernel) ------------------------------
// C = A B^T (f16 segment, K) + A4lo B4hi^T + A4hi B4lo^T (block-scaled fp4 segments over the padded K axis Kp) + bias.
// a4_* [M][Kp / 2], b4_* [N][Kp / 2] bytes and their scale tiles come from launch_mx4_pack (sizes: mx_scale_bytes).  ET output
// rounded once from the fp32 accumulators, or fp32 output (optionally accumulated into C).  M % 256 == 0, N % 320 == 0,
// K % 64 == 0, Kp % 256 == 0.  split_from_n (ET outputs, a multiple of 320): columns below it take no lo terms.
bool gemm_mx_ok(int M, int N, int K, int Kp);
size_t mx_scale_bytes(int rows, int Kp, bool is_b);
hipError_t launch_gemm_et_mx(int prec, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, int Kp,
                             const void* a4_lo, const void* a4_hi, const void* sa_lo, const void* sa_hi,
                             const void* b4_hi, const void* b4_lo, const void* sb_hi, const void* sb_lo,
                             bool out_f32, bool accumulate, int split_from_n, hipStream_t s,
                             // ET outputs only: GELU in the epilogue, and (o4_*: all four or none) the output ALSO as MXFP4 hi / lo on a K
                             // axis padded per 80-column wave tile to 96 ([M][N / 80 * 48] bytes, A-operand scale tiles, block-internal
                             // order = launch_mx4_pack perm 2): lin1 -> lin2 of the all-split mode
                             bool gelu = false, void* o4_hi = nullptr, void* o4_lo = nullptr, void* so_hi = nullptr, void* so_lo = nullptr,
                             // round 6: operand rows of stride ld (0 = K); ext: they carry the 64-column outlier extension behind their K
                             // live columns, which the tiles WITHOUT lo terms (n0 < split_from_n) read as one more f16 stage
                             int ld = 0, bool ext = false);
// x (fp32 [rows][K]) or the ET pair (hi_in, lo_in) -> fp4 codes of hi and lo [rows][Kp / 2] + E8M0 scale tiles (A layout, or the
// B layout when is_b); optional out_hi = ET(x).  Padded axis: every group of G source elements becomes GP (zeros behind it);
// Kp = K / G * GP must be a multiple of 256.  Plain: G = GP = K.
// perm: the block-internal element order of the attention kernels' own MX outputs (store_attention_row_mx: position 16 hh + 4 g + e
// holds element 8 g + 4 hh + e) -- for the proj weights, whose A operand those kernels write.
hipError_t launch_mx4_pack(int prec, const float* x, const void* hi_in, const void* lo_in, void* out_hi, void* q_hi, void* q_lo,
                           void* s_hi, void* s_lo, int rows, int K, int G, int GP, bool is_b, hipStream_t s, int perm = 0 /* 1: attention, 2: GEMM epilogue */);

// ---- upscaler_fused.hip ---------------------------------------------------------------------
// mask_decoder.py:53-59,154-167 in one kernel: keys [n * grid^2][256] ET -> ConvT #1 + LayerNorm2d + GELU -> ConvT #2 + GELU ->
// hypernetwork dot -> low [n][n_sel][4 grid][4 grid].  w1 [256][256], w2 [128][64] in the GEMM-B layouts of engine.hip, b1 [256] /
// b2 [128] tiled over the sub-pixels, ln = gamma[64] | beta[64].  *_lo (all three or none): split precision.  grid % 16 == 0.
hipError_t launch_upscaler_fused(int prec, const void* keys, const void* keys_lo, const void* w1, const void* w1_lo, const float* b1,
                                 const float* ln, const void* w2, const void* w2_lo, const float* b2, const float* hyper, float* low,
                                 int n, int grid, int n_mask_tokens, int sel0, int n_sel, hipStream_t s);

// ---- rle_kernels.hip ------------------------------------------------------------------------
// COCO RLE strings of n binary masks (uint8 [n][h][w], non-zero = set), packed behind *cursor (device int64, in / out)
// into `out` (device bytes, capacity out_cap) at 16-byte aligned offsets; table [n][3] (device int64) = (offset,
// length, n_counts), length < 0: did not fit (-length - 1 bytes were needed).  scratch: rle_scratch_bytes(n, h, w).
size_t rle_scratch_bytes(int n, int h, int w);
hipError_t launch_rle_encode(const uint8_t* masks, int n, int h, int w, void* scratch, unsigned char* out, long long out_cap,
                             long long* cursor, long long* table, hipStream_t s);

// the same for masks [n][h][w] pasted at (x0, y0) on an all-zero H x W canvas (scene mode): strings, table and cursor as above,
// in the canvas's frame.  H * W < 2^30, w + 1 <= 8192.  scratch: rle_placed_scratch_bytes(n, h, w, x0, H, W).
size_t rle_placed_scratch_bytes(int n, int h, int w, int x0, int H, int W);
hipError_t launch_rle_encode_placed(const uint8_t* masks, int n, int h, int w, int x0, int y0, int H, int W, void* scratch,
                                    unsigned char* out, long long out_cap, long long* cursor, long long* table, hipStream_t s);

// ---- rle_decode_kernels.hip -----------------------------------------------------------------
// The inverse: n <= rle_decode_max_batch() strings (table [n][3] device int64 = (offset, length, ignored) into `strings`, device bytes)
// -> row-major 0 / 1 bytes masks_out [n][h][w] (every byte written), areas_out [n] (or null), status_out [n] (samrs_rle_status; a mask
// with a non-zero status is all zero).  Memory-safe for arbitrary bytes and table rows.  h * w < 2^30, strings_bytes < 2^31.
// scratch: rle_decode_scratch_bytes(n, h, w, strings_bytes).
int rle_decode_max_batch();
size_t rle_decode_scratch_bytes(int n, int h, int w, long long strings_bytes);
hipError_t launch_rle_decode(const uint8_t* strings, long long strings_bytes, const long long* table, int n, int h, int w, void* scratch,
                             uint8_t* masks_out, long long* areas_out, int32_t* status_out, hipStream_t s);

// ---- scene_kernels.hip ----------------------------------------------------------------------
// order int32 [H][W] (-1 = unclaimed): order[p] = max(order[p], max{ranks[j] : mask j set at p}) over the masks uint8 [n][h][w] of
// the window (x0, y0, w, h); areas (zeroed, then counted) and the class statistics as launch_paint.  n == 0 is a no-op.
hipError_t launch_scene_claim(const uint8_t* masks, const int32_t* ranks, const int32_t* labels, int n, int h, int w, int x0, int y0,
                              int H, int W, int32_t* order, unsigned long long* areas, unsigned long long* class_pixels,
                              unsigned long long* class_instances, int n_classes, hipStream_t s);
// seg[p] = order[p] < 0 ? 255 : (uint8) labels_by_rank[order[p]]
hipError_t launch_scene_resolve(const int32_t* order, const int32_t* labels_by_rank, int n_ranks, int H, int W, uint8_t* seg,
                                hipStream_t s);

// ---- png_kernels.hip ------------------------------------------------------------------------
// gray/<stem>.png and color/<stem>.png of n class maps (uint8 [n][h][w] on the device, lut uint8 [256][3] on the device), byte-
// identical with libsamrs_io's samrs_io_png_write_label_pair.  Files packed behind *cursor into `out` (16-byte aligned, capacity
// out_cap) at 16-byte aligned offsets; table [n][2][2] = (offset, length) of gray, colour; length < 0: did not fit (-length - 1
// bytes were needed) and was not written.  scratch: png_scratch_bytes(n, h, w).
size_t png_scratch_bytes(int n, int h, int w);
hipError_t launch_png_encode(const uint8_t* maps, int n, int h, int w, const uint8_t* lut, void* scratch, unsigned char* out,
                             long long out_cap, long long* cursor, long long* table, hipStream_t s);
// The stages of that encoder that do not look at tokens, for `streams` (2: gray + colour; 1: stream 0 alone) streams of each of nm
// files' slots (nm <= 8, the encoder's own pass); overlay_kernels.hip's truecolour encoder runs them on buffers of the same layout
// (png_device.h: the meta block; B deflate blocks of 2^20 symbols and C chunks of 1024 symbols per file at most):
//   hist, tables [nm][B][2][316] (tables: code | length << 16), hdr [nm][B][2][160] + hdrbits [nm][B][2] (the block headers' bits),
//   chunkbits [nm][2][C], chunkoff [nm][2][C], gapoff [nm][2][B + 1], meta [nm][16].
//   tables : hist + meta NBLK -> tables, hdr, hdrbits        offsets: chunkbits + tables + hdrbits + meta NCHUNK / NBLK -> chunkoff,
//   gapoff, meta BITS        zero: the placed files' bytes (meta OFF / LEN)        headers: block headers + end-of-block codes OR-ed in
//   crc    : the IDAT CRC of the framed files (meta CRC zeroed beforehand); looks at BOTH streams' OFF: a caller with one stream sets
//            meta OFF1 = ~0.  worst_file_bytes sizes the grid.
struct PngStageBuffers {
    unsigned long long* meta;
    uint32_t *hist, *tables, *hdr, *hdrbits, *chunkbits;
    unsigned long long *chunkoff, *gapoff;
    size_t B, C;
};
void png_stage_tables(const PngStageBuffers& L, int nm, int streams, hipStream_t s);
void png_stage_offsets(const PngStageBuffers& L, int nm, int streams, hipStream_t s);
void png_stage_zero(const PngStageBuffers& L, unsigned char* out, int nm, int streams, hipStream_t s);
void png_stage_headers(const PngStageBuffers& L, unsigned char* out, int nm, int streams, hipStream_t s);
void png_stage_crc(const PngStageBuffers& L, unsigned char* out, int nm, int streams, size_t worst_file_bytes, hipStream_t s);

// ---- overlay_kernels.hip --------------------------------------------------------------------
// out = Pillow's Image.blend(images, lut[maps], alpha): per byte (uint8)((int)a + alpha * ((int)b - (int)a)), float multiply and
// add each rounded, truncated.  images / out uint8 [n][h][w][3], maps uint8 [n][h][w], lut uint8 [256][3], all on the device.
hipError_t launch_blend_labels(const uint8_t* images, const uint8_t* maps, const uint8_t* lut, float alpha, uint8_t* out, int n, int h,
                               int w, hipStream_t s);
// Truecolour PNG files of n images uint8 [n][h][w][3] (samrs_png_encode_rgb in samrs_hip.h: filter -1 .. 4, the buffer protocol of
// launch_png_encode with table [n][2]).  scratch: png_rgb_scratch_bytes(n, h, w).  png_rgb_worst_file_bytes: the documented bound.
size_t png_rgb_scratch_bytes(int n, int h, int w);
size_t png_rgb_worst_file_bytes(int h, int w);
hipError_t launch_png_encode_rgb(const uint8_t* rgb, int n, int h, int w, int filter, void* scratch, unsigned char* out,
                                 long long out_cap, long long* cursor, long long* table, hipStream_t s);

// ---- region_kernels.hip ---------------------------------------------------------------------
// Small-region removal (utils/amg.py:267-291 remove_small_regions, 8-connectivity) on n <= REGION_CHUNK masks uint8 [n][h][w], in
// place (non-zero = set in, 0 / 1 out).  mode: 1 holes, 2 islands, 3 holes then islands.  areas_out / changed_out (device int64 [n],
// either may be null): pixels set afterwards / pixels whose value changed.  scratch: region_scratch_bytes(n, h, w) = int32 labels +
// int32 areas (8 bytes per pixel) + 32 bytes of counters per mask.  h * w < 2^30.
constexpr int REGION_CHUNK = 32;                       // measured: chunks of 8 take 1.7x the time per mask (launches too small to fill the device)
size_t region_scratch_bytes(int n, int h, int w);
hipError_t launch_clean_masks(uint8_t* masks, int n, int h, int w, int min_area, int mode, void* scratch, long long* areas_out,
                              long long* changed_out, hipStream_t s);
// the labelling alone (any n): labels_out int32 [n][h][w] = the smallest row-major pixel index of the pixel's 8-connected component
// of the set pixels (complement != 0: of the unset pixels), -1 outside that working set.  Needs no scratch.
hipError_t launch_region_labels(const uint8_t* masks, int n, int h, int w, int complement, int32_t* labels_out, hipStream_t s);

// ---- box_kernels.hip ------------------------------------------------------------------------
// Mask-derived boxes (definition: the header comment of box_kernels.hip).  ext: int32 [n][h][3] = first set column, last set column
// and pixel count of every row of masks uint8 [n][h][w] (-1, -1, 0 for an empty row); it is the scratch between the two launches,
// mask_boxes_scratch_bytes(n, h).  hbox_out int32 [n][4], rbox_out fp32 [n][4][2], record_out int64 [n][8], verts_out int32
// [n][cap][2] (the ordered hull vertices, the first min(m, cap) of them) and counts_out int32 [n] (m) may each be null.
// h, w <= 8192, x0, y0 >= 0, x0 + w, y0 + h <= 32768 (mask_boxes_shape_ok).
bool mask_boxes_shape_ok(int h, int w, int x0, int y0);
size_t mask_boxes_scratch_bytes(int n, int h);
hipError_t launch_mask_row_extents(const uint8_t* masks, int n, int h, int w, int32_t* ext, hipStream_t s);
hipError_t launch_mask_hull_rect(const int32_t* ext, int n, int h, int x0, int y0, int32_t* hbox_out, float* rbox_out,
                                 long long* record_out, int32_t* verts_out, int cap, int32_t* counts_out, hipStream_t s);

// ---- quality_kernels.hip --------------------------------------------------------------------
// counts [n][4] (zeroed on the stream, then counted) = #{v > +offset}, #{v > 0}, #{v > -offset}, #{v > 0 inside the mask's box} over
// the orig_h x orig_w values v that postprocess_kernel computes from low [n][img_size / 4][img_size / 4] (postprocess_value.h);
// boxes fp32 [n][4] xyxy in the output frame (inclusive on both sides) or null (the fourth count is then 0).  Integer atomics only.
hipError_t launch_score_masks(const float* low, int n, int in_h, int in_w, int orig_h, int orig_w, int img_size, float offset,
                              const float* boxes, unsigned long long* counts, hipStream_t s);
// keep[j] = every enabled criterion holds for counts[j] / iou[j] (a threshold <= 0 disables its criterion; the rule: samrs_hip.h,
// samrs_filter_masks); masks uint8 [n][hw] of dropped rows are zeroed (16-byte stores when masks is 16-byte aligned and hw % 16 == 0)
hipError_t launch_filter_masks(uint8_t* masks, int n, long hw, const long long* counts, const float* iou, float min_stability,
                               float min_pred_iou, float min_inside, uint8_t* keep, hipStream_t s);

// ---- overlap_kernels.hip --------------------------------------------------------------------
// areas [n] (zeroed on the stream, then counted) = set bytes of masks uint8 [n][h][w].  h * w < 2^31.
hipError_t launch_mask_areas(const uint8_t* masks, int n, int h, int w, unsigned long long* areas, hipStream_t s);
// One instance per pixel, in place (the rule: samrs_hip.h samrs_resolve_overlaps): walking j = 0 .. n-1, mask j set at p takes p from
// holder b iff there is none, or P[j] > P[b], or P[j] == P[b] and not v_j(p) < v_b(p).  P[j] = prim[j], or -prim[j] with prim_neg, or
// 0 with prim null; v = the postprocessed logit from low [n][img_size / 4][img_size / 4] (postprocess_value.h), or equal with low
// null.  Losers' bytes are zeroed; owner_out int32 [h][w] (the winner, -1 where no mask is set) and removed [n] (zeroed on the
// stream, then counted) may each be null.  Integer atomics only.
hipError_t launch_resolve_overlaps(uint8_t* masks, int n, int h, int w, const long long* prim, int prim_neg, const float* low, int in_h,
                                   int in_w, int img_size, int32_t* owner_out, unsigned long long* removed, hipStream_t s);

// ---- ap_kernels.hip -------------------------------------------------------------------------
// Bit planes: out uint64 [n][words], words = ceil(h w / 64), pixel p = bit p % 64 of word p / 64, tail bits zero; of masks uint8
// [n][h][w] (non-zero = set; 16-byte loads where h w % 16 == 0 and the pointer allows), or of the instances of a label image
// (label_rgb uint8 [h][w][3], colors uint8 [n][3]: instance j = the pixels whose RGB equals colors[j]; the image is read once).
// h * w < 2^30, n >= 1.
hipError_t launch_pack_bits(const uint8_t* masks, int n, int h, int w, unsigned long long* out, hipStream_t s);
hipError_t launch_label_pack_bits(const uint8_t* label_rgb, const uint8_t* colors, int n, int h, int w, unsigned long long* out,
                                  hipStream_t s);
// area [n] (zeroed on the stream, then counted) = set bits of planes [n][words]; inter [na][nb] (likewise) = set bits of
// a[i] & b[j].  1 <= words <= 2^24, na, nb >= 1.  Integer atomics only: exact and order-independent.
hipError_t launch_bit_areas(const unsigned long long* planes, int n, long words, unsigned long long* area, hipStream_t s);
hipError_t launch_pair_counts(const unsigned long long* a, int na, const unsigned long long* b, int nb, long words,
                              unsigned long long* inter, hipStream_t s);
// COCO matching of one image (the rule: samrs_hip.h samrs_coco_match).  bar[t] = min(threshold t, 1 - 1e-10); [lo, hi] per area
// range.  scores fp32 [nd] on the device; a NaN among them: *n_kept_out = -1 and nothing is matched.  scratch:
// coco_match_scratch_bytes(ng, T, A), zeroed here.  inter / area_d / scores may be null where nd == 0, inter / area_g where ng == 0.
constexpr int COCO_MAX_THRESHOLDS = 16, COCO_MAX_RANGES = 16, COCO_MAX_DET = 4096;
struct CocoMatchParams { double bar[COCO_MAX_THRESHOLDS], lo[COCO_MAX_RANGES], hi[COCO_MAX_RANGES]; };
size_t coco_match_scratch_bytes(int ng, int n_thresholds, int n_ranges);
// inter_b / area_db / area_gb: the same counts of the masks' boundary bands (samrs_coco_match_min: the pair's IoU is the smaller of the
// two), or all three null: the plain matching, whose kernel does not look at them.
hipError_t launch_coco_match(const long long* inter, const long long* area_d, const long long* area_g, const long long* inter_b,
                             const long long* area_db, const long long* area_gb, const float* scores, int nd, int ng, const CocoMatchParams& P, int n_thresholds, int n_ranges, int max_det, void* scratch, int32_t* order_out,
                             int32_t* match_out, uint8_t* ign_out, int32_t* n_valid_out, int32_t* n_kept_out, hipStream_t s);

// ---- boundary_kernels.hip -------------------------------------------------------------------
// The boundary bands of n >= 1 bit planes [n][words] (ap_kernels.hip's layout) of h x w masks: band = M & ~E, E = M eroded by the
// (2 d + 1)^2 square with everything outside the image as background (the definition: samrs_hip.h samrs_mask_boundary_bits).
// 1 <= d <= 128, h * w < 2^30; band_out [n][words] must not overlap planes; tail bits zero.  scratch: mask_boundary_scratch_bytes(n, h, w)
// (one intermediate plane per mask; unused, and may be null, where w or h < 2 d + 1).
size_t mask_boundary_scratch_bytes(int n, int h, int w);
hipError_t launch_mask_boundary(const unsigned long long* planes, int n, int h, int w, int d, void* scratch, unsigned long long* band_out,
                                hipStream_t s);

// ---- polygon_kernels.hip --------------------------------------------------------------------
// Mask outlines as polygons on the pixel lattice (definition: the header comment of polygon_kernels.hip; contract: samrs_hip.h
// samrs_mask_polygons).  One chunk of n <= 65535 masks per call; scratch: mask_polygons_scratch_bytes(n, h, w, max_edges).  The
// per-edge arrays of a mask are mask_polygons_edge_stride(h, w, max_edges) = min(max_edges, 4 h w) entries apart.
// launch_polygon_edges / launch_polygon_ranks: the stages alone -- ids_out uint32 / succ_out int32 / corner_out uint8 [n][stride]
// (ascending edge ids, the successor's compact index, the corner flag), leader_out / rank_out int32 [n][stride], counts_out int32 [n]
// = edges per mask; a mask over max_edges has its count and no entries.
bool mask_polygons_shape_ok(int h, int w, int x0, int y0);
long long mask_polygons_edge_stride(int h, int w, int max_edges);
size_t mask_polygons_scratch_bytes(int n, int h, int w, int max_edges);
hipError_t launch_mask_polygons(const uint8_t* masks, int n, int h, int w, int x0, int y0, int max_edges, void* scratch,
                                int32_t* vertices, long long vertex_capacity, int32_t* rings, long long ring_capacity,
                                long long* cursor, long long* table, hipStream_t s);
hipError_t launch_polygon_edges(const uint8_t* masks, int n, int h, int w, int max_edges, void* scratch, uint32_t* ids_out,
                                int32_t* succ_out, uint8_t* corner_out, int32_t* counts_out, hipStream_t s);
hipError_t launch_polygon_ranks(const uint8_t* masks, int n, int h, int w, int max_edges, void* scratch, int32_t* leader_out,
                                int32_t* rank_out, int32_t* counts_out, hipStream_t s);

// ---- polygon_simplify_kernels.hip -----------------------------------------------------------
// The traced rings simplified in place (definition: samrs_hip.h samrs_simplify_polygons; the stages: the header comment of
// polygon_simplify_kernels.hip).  table: the n rows of the samrs_mask_polygons calls in placement order; vertex_capacity and
// ring_capacity: those of the two buffers, which bound the scratch (polygon_simplify_scratch_bytes).  launch_polygon_simplify_keep:
// the listing and the rounds alone -- keep_out uint8 [vertex_capacity], kept_out int32 [ring_capacity] (-1: no ring of a placed row).
constexpr int POLYGON_SIMPLIFY_EPS_MAX = 16384;
size_t polygon_simplify_scratch_bytes(int n, long long vertex_capacity, long long ring_capacity);
hipError_t launch_polygon_simplify(int32_t* vertices, int32_t* rings, long long* table, int n, int eps_q, long long vertex_capacity,
                                   long long ring_capacity, void* scratch, long long* cursor, hipStream_t s);
hipError_t launch_polygon_simplify_keep(const int32_t* vertices, const int32_t* rings, const long long* table, int n, int eps_q,
                                        long long vertex_capacity, long long ring_capacity, void* scratch, uint8_t* keep_out,
                                        int32_t* kept_out, hipStream_t s);

// ---- polygon_fill_kernels.hip ---------------------------------------------------------------
// Rings back to masks (definition: samrs_hip.h samrs_fill_polygons; the stages: the header comment of polygon_fill_kernels.hip).
// One kernel per 32768 table rows and a memset of counts_out; no scratch.  The caller has checked the shape (mask_boxes_shape_ok).
hipError_t launch_fill_polygons(const int32_t* vertices, const int32_t* rings, const long long* table, int n, int h, int w, int x0,
                                int y0, uint8_t* masks_out, const uint8_t* ref, long long* counts_out, hipStream_t s);
