/*
 * samrs_hip_internal.h -- NOT the drop-in boundary.  Kernel-level entry points (samrs_k_*: one kernel each, used by the parity
 * tests to check every kernel alone against the oracle) and test / measurement hooks (samrs_debug_*) of libsamrs_hip.so.
 * A caller that binds the engine (include/samrs_hip.h) needs nothing from this file; nothing here carries a
 * compatibility promise, and several entries keep process-wide or per-device state that product code must not share
 * (noted at each).  VERDICT r05 "what's weak" 12: a caller linking the public header could not tell product from probe.
 */
#ifndef SAMRS_HIP_INTERNAL_H
#define SAMRS_HIP_INTERNAL_H

#include "samrs_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* -- test hook: run preprocess + patch embed + the first n_blocks encoder blocks for n_images
 * tiles and copy the fp32 residual stream [n_images*4096, embed_dim] (channels-last,
 * image_encoder.py:107-112) to x_out.  Invalidates the embedding slots. */
int samrs_debug_encoder_prefix(samrs_engine_t* e, const uint8_t* images, int n_images, int in_h,
                               int in_w, int n_blocks, float* x_out, void* stream);

/* -- test hook: the outlier K-columns (option "outlier_cols") picked at samrs_finalize_weights for block GEMM `gemm` (0 qkv, 1 lin1,
 * 2 lin2, 3 proj) of encoder block `block`: returns their number (<= 32) and writes the ascending indices to the HOST array out32. */
int samrs_debug_outlier_columns(samrs_engine_t* e, int block, int gemm, int32_t* out32);

/* -- process-wide test / tuning hooks of the KERNEL-LEVEL entry points below (samrs_k_gemm has no handle): GEMM tile variant,
 * and the start skew of the first round of GEMM blocks, per XCD / per CU group, in 1024-cycle units (0, 0 = off). */
void samrs_debug_set_gemm_variant(int variant);
/* -- probe, no HIP call: which kernel a samrs_k_gemm call of this shape and these flags would run under `variant` (8 = automatic; the
 * SAMRS_GEMM_W4X / SAMRS_GEMM_M32 switches of the process apply).  has_add2d: a 2-D addend is given; ld: operand row stride, 0 = K (the
 * engine's padded qkv / lin1 operands).  out[8] = enum GemmKernel of csrc/gemm_select.h, ni, mode, persistent, reject (1 = the call
 * returns an error with nothing launched), then what the engine's three planning questions answer for (M, N, K, gelu) under the same
 * variant: operands may be padded (a plain ET launch runs on a kernel that takes `ld`), the outlier-column stage fits, the LayerNorm
 * tail fits. */
void samrs_debug_gemm_choice(int prec, int M, int N, int K, int out_f32, int gelu, int accumulate, int has_add2d, int ld, int variant,
                             int32_t* out);
void samrs_debug_set_gemm_skew(int xcd_units, int cu_units);
/* 1 when the library was built with `make EXPERIMENTS=1`: the kernels that were measured and not adopted (GEMM variants 30 - 36 on
 * v_mfma_f32_32x32x16, the LayerNorm fold "ln_fold", the timing ablations 60 - 92 / 100 - 196) exist; 0 in the product build, where those
 * variants fall back to the default kernels and "ln_fold" = 1 is refused. */
int samrs_debug_has_experiments(void);

/* -- test hook: copy a prefix of a named internal decoder buffer (Q, KF, KE, KVQ, OI, U1raw, U1, U2,
 * HYPER, TOK0, K0F, DENSE, ...) to a device buffer; used to localise run-to-run differences and by the stage-by-stage decoder
 * test.  A buffer that does not exist yet (DENSE before the first mask prompt, any name before samrs_finalize_weights) is an
 * error, not a copy from a null pointer. */
int samrs_debug_copy_buffer(samrs_engine_t* e, const char* name, void* dst, size_t bytes, void* stream);

/* -- measurement hook: when enabled, samrs_set_images brackets every launch of the dominant kernel
 * (MLP lin1 + GELU GEMM, [n*4096, D] x [4D, D]^T) with hipEvents on the launch stream.
 * samrs_debug_dominant_kernel_time() synchronises those events, returns the average duration (ms),
 * the number of launches since the last call, and the GEMM's N / K. */
int samrs_debug_time_dominant_kernel(samrs_engine_t* e, int enable);
int samrs_debug_dominant_kernel_time(samrs_engine_t* e, float* avg_ms, int* launches, int* M, int* N, int* K);

/* -- kernel-level entry points (used by the parity tests to check each kernel alone) --------
 * All pointers are device pointers.  `prec` is enum samrs_precision; "et" = MFMA operand type
 * (bf16 or f16 bit patterns in uint16). */
int samrs_k_gemm(int prec, const void* A_et, const void* B_et, void* C, const float* bias,
                 const float* add2d, int add2d_period, int M, int N, int K,
                 int out_f32, int gelu, int accumulate, void* stream);
int samrs_k_gemm_f32(const float* A, int lda, const float* W, const float* bias, float* C, int ldc,
                     int M, int N, int K, int relu, int accumulate, void* stream);
/* LayerNorm folded into the neighbouring GEMMs of an encoder block (image_encoder.py:168,177; residual stream of 1280 columns):
 *   samrs_k_gemm_stats       C (fp32) += A_et B_et^T + bias;  xh_et = ET(C);  stats[m][8] = (mean, sum of squared deviations)
 *                            of eight 160-element groups of row m.  M % 256 == 0, N == 1280, K % 128 == 0.
 *   samrs_k_ln_rowstat       rowstat[m] = (rstd_m, -rstd_m mean_m) merged from stats[m][.] with eps
 *   samrs_k_gemm_fold        C_et = [GELU](rstd_m (xh_et Wf_et^T - mean_m cvec) + bias_f) with rowstat from above.
 *                            M % 256 == 0, N % 320 == 0, K == 1280.
 *   samrs_k_ln_fold_weight   Wf_et = ET(W diag(gamma)), cvec[n] = sum_k Wf_et[n][k], bias_f = bias + W beta  (W fp32 [N][K])
 *   samrs_k_rowstats_convert xh_et = ET(X), stats as above, for X fp32 [rows][1280] */
int samrs_k_gemm_stats(int prec, const void* A_et, const void* B_et, float* C, const float* bias, void* xh_et, float* stats,
                       int M, int N, int K, void* stream);
int samrs_k_ln_rowstat(const float* stats, float* rowstat, int rows, float eps, void* stream);
int samrs_k_gemm_fold(int prec, const void* xh_et, const void* Wf_et, void* C_et, const float* bias_f, const float* cvec,
                      const float* rowstat, int M, int N, int K, int gelu, void* stream);
int samrs_k_ln_fold_weight(int prec, const float* W, const float* gamma, const float* beta, const float* bias, void* Wf_et,
                           float* cvec, float* bias_f, int N, int K, void* stream);
int samrs_k_rowstats_convert(int prec, const float* X, void* xh_et, float* stats, int rows, int D, void* stream);
int samrs_k_convert(int prec, const float* in, void* out_et, int64_t n, void* stream);
int samrs_k_layernorm(int prec, const float* X, const float* gamma, const float* beta, float eps,
                      void* out_et, float* out_f32, int rows_out, int D, int window_mode,
                      int n_images, int grid, int window, void* stream);
/* qkv_et: [n_images*grid*grid, 3D] in token order; qkv_bias fp32 [3D] supplies k / v of the window
 * padding positions (zero tokens after norm1 in the reference). */
int samrs_k_window_attention(int prec, const void* qkv_et, const float* qkv_bias, const float* rel_h,
                             const float* rel_w, void* out_et, int n_images, int grid, int window,
                             int heads, int head_dim, void* stream);
/* TEST hook: the same kernel (window 14) with out_lo_et, the split remainder of out_et, written for the heads whose bit is set in
 * lo_heads only (what the engine passes from the outlier columns of proj); rows of the other heads in out_lo_et are left alone. */
int samrs_k_window_attention_lo(int prec, const void* qkv_et, const float* qkv_bias, const float* rel_h, const float* rel_w,
                                void* out_et, void* out_lo_et, int n_images, int grid, int heads, int head_dim, uint32_t lo_heads,
                                void* stream);
/* TEST / BENCH hook (as is samrs_k_attention_mx with global = 1): the V^T workspace the engine owns is, here, one grow-only
 * buffer per device kept by the library; growing it synchronizes the device first.  Not for product code: an engine's own
 * encoder pass (samrs_set_images) uses the engine's workspace and never this one. */
int samrs_k_global_attention(int prec, const void* qkv_et, const float* rel_h, const float* rel_w,
                             void* out_et, int n_images, int grid, int heads, int head_dim,
                             void* stream);
/* neck (image_encoder.py:88-104): im2col of the 3x3 / pad 1 convolution on a channels-last ET tensor
 * in [n_images][grid][grid][C] -> A [n_images*grid*grid][9*C], k = (ky*3 + kx)*C + c, zero outside the image. */
int samrs_k_neck_im2col(const void* in_et, void* A_et, int n_images, int grid, int C, void* stream);
int samrs_k_postprocess(const float* lowres, int n_masks, int in_h, int in_w, int orig_h,
                        int orig_w, int img_size, int return_logits, void* out, void* stream);
/* First transposed conv of the mask upscaler as a GEMM with LayerNorm2d(64) + GELU in its epilogue
 * (segment_anything/modeling/mask_decoder.py:53-56): C_et[M,N] = GELU(LN64(A_et[M,K] B_et[N,K]^T + bias)),
 * every 64-column group of N normalised on its own, eps 1e-6; gamma_beta = gamma[64] | beta[64].
 * M % 256 == 0, N % 128 == 0, K % 32 == 0.  A_lo_et / B_lo_et (both or neither; samrs_k_convert_split): the split
 * remainders of the operands -- the product then runs as A_lo B + A B_lo + A B and C is written in FP32 [M][N].
 * This hook and the two below (tests/test_upscaler_kernels_gpu.py) check on the host what the engine's call sites guarantee and
 * launch nothing otherwise: SAMRS_ERR_BAD_ARG for a prec that is neither type, a null required pointer (bias and gamma_beta
 * included), a pointer that is not 16-byte aligned, lo operands given in part; SAMRS_ERR_BAD_SHAPE for M, N, K outside the above. */
int samrs_k_gemm_gln(int prec, const void* A_et, const void* B_et, void* C_et, const float* bias,
                     const float* gamma_beta, int M, int N, int K, const void* A_lo_et, const void* B_lo_et, void* stream);
/* Split-precision GEMM in one launch (the block GEMMs of the reference-grade mode, option "split" bits 16 / 32):
 * C = A B^T + A_lo B^T + A B_lo^T + bias over a three-segment K axis; A*, [M,K], B*, [N,K] in the operand type (hi / lo from
 * samrs_k_convert_split).  out_f32 = 0: C_et [M,N] rounded once from the fp32 accumulators; out_f32 = 1: C fp32 [M,N],
 * accumulate != 0 adds to what C holds (the residual stream).  M % 256 == 0, N % 320 == 0, K % 64 == 0, else SAMRS_ERR_BAD_SHAPE.
 * split_from_n (out_f32 = 0 only, a multiple of 320, 0 = everywhere): only output columns >= split_from_n take the lo terms. */
int samrs_k_gemm_split3(int prec, const void* A_et, const void* A_lo_et, const void* B_et, const void* B_lo_et, void* C,
                        const float* bias, int M, int N, int K, int out_f32, int accumulate, int split_from_n, void* stream);
/* Second transposed conv + GELU + hypernetwork product (mask_decoder.py:57-59,154-167) in one pass:
 * u1_et [n*grid*grid*4, 64] (rows = prompt, token, sub-pixel 1), w_et [128, 64] (rows = sub-pixel 2 x 32
 * channels), bias [128], hyper [n, n_mask_tokens, 32] -> low [n, n_sel, 4*grid, 4*grid] fp32 for mask
 * tokens sel0 .. sel0+n_sel-1 (n_sel 1 or 3).  grid*grid*4 % 1024 == 0.  w_lo_et != NULL: split precision -- u1 is then
 * FP32 [rows][64] (split into hi + lo in registers) and w_lo_et the remainder of the weight split.
 * SAMRS_ERR_BAD_SHAPE, nothing launched: n < 1, grid < 16 or not a multiple of 16 (or > 1024), n_mask_tokens < 1, sel0 < 0,
 * n_sel not 1 or 3, sel0 + n_sel > n_mask_tokens (the last prompt's rows would be read past hyper). */
int samrs_k_upscale2_masks(int prec, const void* u1, const void* w_et, const void* w_lo_et, const float* bias,
                           const float* hyper, float* low, int n, int grid, int n_mask_tokens,
                           int sel0, int n_sel, void* stream);
/* The whole mask upscaler in one kernel (mask_decoder.py:53-59,154-167): keys_et [n*grid*grid, 256] -> ConvT #1 (w1_et [256][256]
 * rows = sub-pixel 1 x 64 channels, b1 [256]) -> LayerNorm2d(64) (ln = gamma[64] | beta[64], eps 1e-6) -> GELU -> ConvT #2
 * (w2_et [128][64] rows = sub-pixel 2 x 32 channels, b2 [128]) -> GELU -> dot with hyper [n, n_mask_tokens, 32] ->
 * low [n, n_sel, 4*grid, 4*grid] fp32.  keys_lo / w1_lo / w2_lo (all three or none): split precision.  grid % 16 == 0.
 * The same argument and shape checks as samrs_k_upscale2_masks; every pointer, low included, 16-byte aligned. */
int samrs_k_upscaler_fused(int prec, const void* keys_et, const void* keys_lo_et, const void* w1_et, const void* w1_lo_et,
                           const float* b1, const float* ln, const void* w2_et, const void* w2_lo_et, const float* b2,
                           const float* hyper, float* low, int n, int grid, int n_mask_tokens, int sel0, int n_sel, void* stream);
/* -- prompt encoder and two-way transformer glue (decoder_kernels.hip), one kernel each; tests/test_decoder_kernels_gpu.py.
 * None takes an engine handle: the weights arrive as pointers.  A shape the launcher does not cover returns non-zero with
 * nothing launched.
 *   samrs_k_prompt_tokens   tokens [n][T][256] (and the same bits to tokens2 when given) = iou token | 4 mask tokens | points
 *                           (+ one pad point when there is no box) | 2 box corners; T = 5 + n_points (+ 1) (+ 2), checked.
 *                           boxes [n][4] / point_coords [n][n_points][2] / point_labels int32 [n][n_points] (either group or both);
 *                           gauss [2][128], point_emb [4][256], not_a_point / iou_token [256], mask_tokens [4][256].
 *   samrs_k_dense_pe        pe [grid * grid][256]
 *   samrs_k_mask_embed      mask_in [n][4 grid][4 grid] -> dense [n][grid * grid][256]; conv 2x2/2 (w0 [4][1][2][2]) + LN2d(4) + GELU,
 *                           conv 2x2/2 (w3 [16][4][2][2]) + LN2d(16) + GELU, conv 1x1 (w6 [256][16]).  grid * grid % 16 == 0.
 *   samrs_k_fill_slot_table out[p] = slot[k] for start[k] <= p < start[k + 1], k < n_runs; start / slot are HOST arrays
 *   samrs_k_make_keys       out_f32 / out_et [n_batches][tokens][C] = emb[slot_of ? slot_of[b] : 0] + (dense ? dense[b] : vec[C])
 *   samrs_k_token_self_attn q, k, v, o fp32 [n][T][C], head dim 32, T <= 16
 *   samrs_k_t2i_attention   qp fp32 [n][T][128]; kp / vp ET rows of ld elements, batch bstride rows apart (slot_of: batch slot_of[b]);
 *                           out fp32 [n][T][128]; workspace of samrs_k_t2i_workspace_floats(n, T) floats.  T <= 16.
 *   samrs_k_i2t_attention   qi ET rows of ld elements (batch stride bstride rows); kt, vt fp32 [n][T][128]; out ET [n][tokens][128]
 *   samrs_k_i2t_fused       LayerNorm(resid + out_proj(that attention)) -> outF fp32 (optional), outE, outE_lo (optional)
 *                           [n][tokens][256]; w (w_lo: split) ET [256][128]; resid fp32 rows of 256, batch stride r_bstride rows;
 *                           slot_of strides the query and the residual.  tokens % 32 == 0, 1 <= T <= 16.
 *   samrs_k_group_ln_gelu   in fp32 [rows][4 * 64] -> LayerNorm per 64-group (gamma, beta [64]) + GELU -> out ET
 *   samrs_k_mask_product    up2 ET [n * grid^2 * 16][32], hyper [n][n_mask_tokens][32] -> low [n][n_sel][4 grid][4 grid], n_sel <= 4 */
int samrs_k_prompt_tokens(const float* boxes, const float* point_coords, const int32_t* point_labels, int n_prompts, int n_points,
                          float img_size, const float* gauss, const float* point_emb, const float* not_a_point, const float* iou_token,
                          const float* mask_tokens, float* tokens, float* tokens2, int T, void* stream);
int samrs_k_dense_pe(const float* gauss, float* pe, int grid, void* stream);
int samrs_k_mask_embed(const float* w0, const float* b0, const float* ln1w, const float* ln1b, const float* w3, const float* b3,
                       const float* ln4w, const float* ln4b, const float* w6, const float* b6, const float* mask_in, float* dense,
                       int n, int grid, void* stream);
int samrs_k_fill_slot_table(const int32_t* start_host, const int32_t* slot_host, int n_runs, int32_t* out, void* stream);
int samrs_k_make_keys(int prec, const float* emb, const float* dense, const float* vec, float* out_f32, void* out_et, int n_batches,
                      int tokens, int C, const int32_t* slot_of, void* stream);
int samrs_k_token_self_attn(const float* q, const float* k, const float* v, float* o, int n, int T, int C, int heads, void* stream);
int64_t samrs_k_t2i_workspace_floats(int n, int T);
int samrs_k_t2i_attention(int prec, const float* qp, const void* kp_et, const void* vp_et, int ld, int64_t bstride, float* out,
                          float* workspace, int n, int T, int tokens, int Ci, int heads, const int32_t* slot_of, void* stream);
int samrs_k_i2t_attention(int prec, const void* qi_et, int ld, int64_t bstride, const float* kt, const float* vt, void* out_et, int n,
                          int T, int tokens, int Ci, int heads, void* stream);
int samrs_k_i2t_fused(int prec, const void* qi_et, int ld, int64_t q_bstride, const float* kt, const float* vt, const void* w_et,
                      const void* w_lo_et, const float* bias, const float* resid, int64_t r_bstride, const float* gamma,
                      const float* beta, float eps, float* outF, void* outE, void* outE_lo, int n, int T, int tokens, int Ci, int C,
                      const int32_t* slot_of, void* stream);
int samrs_k_group_ln_gelu(int prec, const float* in, const float* gamma, const float* beta, float eps, void* out_et, int64_t rows,
                          int groups, int gsize, void* stream);
int samrs_k_mask_product(int prec, const void* up2_et, const float* hyper, float* low, int n, int grid, int n_mask_tokens, int sel0,
                         int n_sel, void* stream);
/* Operand split with the two correction terms on MXFP4 operands (gfx950 v_mfma_scale_f32_16x16x128_f8f6f4, e2m1 codes + one E8M0
 * scale per 32 k; option "lo_format" = 4):
 *   samrs_k_mx4_pack   x (fp32 [rows][K]) or the ET pair (hi_in, lo_in) -> fp4 codes of hi / lo, q_* [rows][Kp / 2] bytes, and their
 *                      scale tiles s_* (samrs_k_mx_scale_bytes(rows, Kp, is_b) bytes each; A-operand or B-operand tile order);
 *                      out_hi (optional, with x): ET(x).  Every group of G source elements becomes GP on the padded axis (zeros
 *                      behind it): Kp = K / G * GP, a multiple of 256; plain: G = GP = K.  is_b: bit 0 = B-operand scale tiles, bit 2 = the block order of a GEMM epilogue's MX rows (position 8 f + 4 i + e holds column 16 i + 4 f + e), bit 1 = the
 *                      block-internal element order in which the attention kernels emit their own MX rows (position 16 h + 4 g + e
 *                      of a block holds element 8 g + 4 h + e): what the proj weights are packed with.
 *   samrs_k_gemm_mx    C = A B^T + A4lo B4hi^T + A4hi B4lo^T + bias: the f16 product over K, the two fp4 products over Kp, fp32
 *                      accumulators throughout; out_f32 = 0: C_et rounded once, = 1: fp32 (accumulate != 0 adds to C).
 *                      M % 256 == 0, N % 320 == 0, K % 64 == 0; split_from_n as for samrs_k_gemm_split3. */
/* the attention kernels with their optional extra outputs: out_lo (the f16 split remainder) or, instead, hi / lo of the output as
 * MXFP4 on the per-head padded K axis (q_* [rows][heads * ceil32(head_dim) / 2], A-operand scale tiles); global = 0: windowed (14) */
int samrs_k_attention_mx(int prec, int global, const void* qkv_et, const float* qkv_bias, const float* rel_h, const float* rel_w,
                         void* out_et, void* out_lo_et, int n_images, int grid, int heads, int head_dim, void* q_hi, void* q_lo,
                         void* s_hi, void* s_lo, void* stream);
int64_t samrs_k_mx_scale_bytes(int rows, int Kp, int is_b);
/* LayerNorm that also emits its output as MXFP4 hi / lo (what the engine feeds the qkv GEMM in "lo_format" 4): D % 256 == 0 */
int samrs_k_layernorm_mx(int prec, const float* X, const float* gamma, const float* beta, float eps, void* out_et, int rows, int D,
                         void* q_hi, void* q_lo, void* s_hi, void* s_lo, void* stream);
int samrs_k_mx4_pack(int prec, const float* x, const void* hi_in, const void* lo_in, void* out_hi, void* q_hi, void* q_lo, void* s_hi,
                     void* s_lo, int rows, int K, int G, int GP, int is_b, void* stream);
int samrs_k_gemm_mx(int prec, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, int Kp, const void* a4_lo,
                    const void* a4_hi, const void* sa_lo, const void* sa_hi, const void* b4_hi, const void* b4_lo, const void* sb_hi,
                    const void* sb_lo, int out_f32, int accumulate, int split_from_n, void* stream);
/* samrs_k_gemm_mx with an ET output, optionally the exact-erf GELU in the epilogue, and (o4_*: all four or none) the output ALSO written
 * as MXFP4 hi / lo on a K axis padded per 80-column wave tile to 96 -- [M][N / 80 * 48] bytes + A-operand scale tiles, block-internal
 * order = samrs_k_mx4_pack is_b bit 2: lin1 feeding lin2 in the all-split mode.  `gelu`: bit 0 = GELU, bit 1 = NO tile takes lo terms
 * (lin1 of split 207, whose lin2 alone is split: the plain persistent kernel with the MX-row epilogue; the a4 / b4 operands are ignored) */
int samrs_k_gemm_mx_gelu_mxout(int prec, const void* A, const void* B, void* C_et, const float* bias, int M, int N, int K, int Kp,
                               const void* a4_lo, const void* a4_hi, const void* sa_lo, const void* sa_hi, const void* b4_hi, const void* b4_lo,
                               const void* sb_hi, const void* sb_lo, int gelu, void* o4_hi, void* o4_lo, void* so_hi, void* so_lo, void* stream);
/* fp32 -> hi (= samrs_k_convert) and lo = ET(x - hi): the two-term operand split */
int samrs_k_convert_split(int prec, const float* in, void* out_hi_et, void* out_lo_et, int64_t n, void* stream);
/* the checkpoint audit's two kernels alone (audit_kernels.hip; row layout and semantics: samrs_hip.h samrs_audit_read_profile).
 *   samrs_k_range_profile  ADDS the profile of x_et -- n elements as rows of `cols` live elements at a row stride of `ld` elements
 *                          (cols <= 0: one dense run; n, cols, ld % 8 == 0, 16-byte aligned) -- into row48 (device int64 [48])
 *   samrs_k_column_stats   x_et [M][K] with row stride ld (K, ld % 8 == 0): sumsq[c] += sum over the rows of x^2 (device double [K]),
 *                          maxbits[c] = max(maxbits[c], bits & 0x7fff) (device uint32 [K]); partials: device fp32 scratch
 *                          [ceil(M / R)][K] with R = samrs_k_audit_rows_per_partial(), the rows one fp32 chain sums before fp64 takes over */
int samrs_k_range_profile(int prec, const void* x_et, long n, int cols, int ld, int64_t* row48, void* stream);
int samrs_k_column_stats(int prec, const void* x_et, int M, int K, int ld, float* partials, double* sumsq, uint32_t* maxbits, void* stream);
int samrs_k_audit_rows_per_partial(void);
/* -- the outlier-column route (option "outlier_cols") and the padded operand rows of the ViT-H block GEMMs, one kernel or launch each;
 * tests/test_outlier_kernels_gpu.py.  Every index array is a DEVICE array of at most 32 distinct, ascending int32 below the column
 * count it indexes; the hooks read it back and refuse anything else (and any shape the launcher does not cover) with nothing launched.
 *   samrs_k_gemm_ld             C_et [M][N] = [GELU](A_et B_et^T + bias) with A, B rows at a stride of ld elements (0 = K): the plain ET
 *                               launch of the engine's qkv / lin1 (kernels.h GemmOpts); gelu_form 1 or 2.  Refused where the selection
 *                               rule does not pick a kernel that takes a stride (samrs_debug_gemm_choice says which).
 *   samrs_k_gemm_ext            C (fp32 [M][N]) += A_et B_et^T + Ax_et Bx_et^T + bias, Ax [M][64], Bx [N][64] dense: proj / lin2 with
 *                               the outlier-column stage; SAMRS_ERR_BAD_SHAPE where the 256 x 320 pair-stage kernel does not take the shape
 *   samrs_k_layernorm_ext       samrs_k_layernorm (plain row order, ET output) into rows of ld_out elements (0 = D) with the extension:
 *                               [D + j] = lo, [D + 32 + j] = hi of column oc_idx[j], j < n_oc; zeros in the unused slots and in
 *                               [D + 64, ld_out).  n_oc > 0 needs ld_out >= D + 64 and window_mode == 0.
 *   samrs_k_outlier_weight_ext  out_et[r][col0 + j] = hi, [col0 + 32 + j] = lo of W[r][idx[j]] (W fp32 [N][K]), rows of ld elements,
 *                               zeros in the unused slots of the 64
 *   samrs_k_outlier_side_weight out_et [32][Ks]: row j < n2 = ET(W1[idx2[j]][0 .. D)) | hi x 32 | lo x 32 of its columns idx1 | zeros;
 *                               rows >= n2 zero; bias_out [32] = b1[idx2[j]] | zeros.  W1 fp32 [n_rows1][D]; Ks >= D (+ 64 when n1 > 0)
 *   samrs_k_outlier_gather      out_et [rows][64]: [j] = lo_et[r][idx[j]], [32 + j] = hi_et[r][idx[j]] (hi, lo [rows][D]), zeros behind n_oc
 *   samrs_k_outlier_side_gemm   out_et [M][64] = lo x 32 | hi x 32 of GELU(Y_et Ws_et^T + bias) before its rounding; Y rows of lda
 *                               elements, Ws [32][K], bias [32]; M % 64 == 0, K % 32 == 0, lda >= K, lda % 8 == 0
 *   samrs_k_weight_norms        col_sq [K] / row_sq [N] (either may be null) = squared L2 norms of the columns / rows of W fp32 [N][K]
 *   samrs_k_range_scan          *counter (device uint64) += the elements of x_et at the operand type's saturation value or beyond; n
 *                               elements as rows of `cols` live elements at a stride of ld (cols <= 0: one dense run); n, cols, ld % 8 == 0 */
int samrs_k_gemm_ld(int prec, const void* A_et, const void* B_et, void* C_et, const float* bias, int M, int N, int K, int ld, int gelu,
                    int gelu_form, void* stream);
int samrs_k_gemm_ext(int prec, const void* A_et, const void* B_et, const void* Ax_et, const void* Bx_et, float* C, const float* bias, int M,
                     int N, int K, void* stream);
int samrs_k_layernorm_ext(int prec, const float* X, const float* gamma, const float* beta, float eps, void* out_et, int rows, int D,
                          int ld_out, const int32_t* oc_idx, int n_oc, int window_mode, void* stream);
int samrs_k_outlier_weight_ext(int prec, const float* W, int N, int K, const int32_t* idx, int n_oc, void* out_et, int ld, int col0,
                               void* stream);
int samrs_k_outlier_side_weight(int prec, const float* W1, const float* b1, int n_rows1, int D, const int32_t* idx2, int n2,
                                const int32_t* idx1, int n1, void* out_et, int Ks, float* bias_out, void* stream);
int samrs_k_outlier_gather(const void* hi_et, const void* lo_et, int D, const int32_t* idx, int n_oc, void* out_et, int rows, void* stream);
int samrs_k_outlier_side_gemm(int prec, const void* Y_et, int lda, const void* Ws_et, const float* bias, int M, int K, void* out_et,
                              void* stream);
int samrs_k_weight_norms(const float* W, int N, int K, float* col_sq, float* row_sq, void* stream);
int samrs_k_range_scan(int prec, const void* x_et, int64_t n, int cols, int ld, uint64_t* counter, void* stream);
/* -- the token side of the mask decoder, image ingest, the embedding hand-over and the reference-grade GELU, one kernel each;
 * tests/test_token_side_kernels_gpu.py.  Each hook repeats on the host what the engine's call sites guarantee by construction and
 * returns SAMRS_ERR_BAD_ARG otherwise, with nothing launched.
 *   samrs_k_gemm_f32_batch  `count` (1 .. 5) fp32 problems of one shape in one launch, as the decoder batches its q / k / v, k / v and head
 *                           GEMMs: C[z] [M][N] (rows of ldc elements) = (A[z] + A2[z]) [M][K] (rows of lda elements) W[z]^T (dense [N][K])
 *                           + bias[z], then ReLU, then + what C[z] held when `accumulate`.  A, A2, W, bias, C are HOST arrays of `count`
 *                           device pointers; A2 may be a null array or hold null entries (no addend for that problem; the sum is rounded
 *                           to fp32 once), bias may hold null entries.  K % 16 == 0, lda % 4 == 0, lda >= K, ldc >= N, M, N >= 1; A[z], A2[z]
 *                           and W[z] 16-byte aligned; A[z], W[z], C[z] non-null.  The bits of a row do not depend on M or on count.
 *   samrs_k_patch_im2col    preprocess + im2col of the patch convolution (sam.py:164-174, image_encoder.py:364-395): img_u8 [n_images][in_h]
 *                           [in_w][3] -> A_et [n_images * grid * grid][3 patch^2], k = c patch^2 + ky patch + kx, value
 *                           (pixel - mean[c]) / std[c] inside in_h x in_w and zero outside; A_lo_et (may be null): the split remainder
 *                           ET(v - hi), same layout.  patch % 8 == 0, in_h, in_w, n_images, grid >= 1, outputs 16-byte aligned.
 *   samrs_k_transpose_f32   out [cols][rows] = in [rows][cols]^T, fp32 bits moved as they are (samrs_get_embedding / samrs_set_embedding)
 *   samrs_k_gelu_split      hi_et | lo_et [n] = the two-term split of the exact-erf GELU of in fp32 [n] (lin1 -> lin2 of the reference-grade
 *                           mode); n % 4 == 0, 16-byte aligned */
int samrs_k_gemm_f32_batch(const float* const* A, const float* const* A2, const float* const* W, const float* const* bias, float* const* C,
                           int count, int lda, int ldc, int M, int N, int K, int relu, int accumulate, void* stream);
int samrs_k_patch_im2col(int prec, const uint8_t* img_u8, void* A_et, void* A_lo_et, int n_images, int in_h, int in_w, int grid, int patch,
                         void* stream);
int samrs_k_transpose_f32(const float* in, float* out, int rows, int cols, void* stream);
int samrs_k_gelu_split(int prec, const float* in, void* hi_et, void* lo_et, int64_t n, void* stream);
/* the connected-component labelling of samrs_clean_masks alone (region_kernels.hip): masks uint8 [n][h][w] (non-zero = set) ->
 * labels_out int32 [n][h][w] = the flattened root of every pixel, i.e. the smallest row-major pixel index of its 8-connected
 * component of the set pixels (complement != 0: of the unset pixels), -1 where the pixel is not in that working set */
int samrs_k_region_labels(const uint8_t* masks, int n, int h, int w, int complement, int32_t* labels_out, void* stream);
/* the two kernels of samrs_mask_boxes alone (box_kernels.hip).
 *   samrs_k_mask_row_extents  ext_out int32 [n][h][3] = first set column, last set column, pixel count of every row (-1, -1, 0 for an
 *                             empty row)
 *   samrs_k_mask_hull         the ordered strict hull vertices: verts_out int32 [n][cap][2] = (x, y) of the first min(m, cap) vertices
 *                             in the frame of (x0, y0), counts_out int32 [n] = m; ext_scratch: device int32 [n][h][3] */
int samrs_k_mask_row_extents(const uint8_t* masks, int n, int h, int w, int32_t* ext_out, void* stream);
int samrs_k_mask_hull(const uint8_t* masks, int n, int h, int w, int x0, int y0, int32_t* ext_scratch, int32_t* verts_out, int cap,
                      int32_t* counts_out, void* stream);
/* the stages of samrs_mask_polygons alone (polygon_kernels.hip), for one chunk of n <= 65535 masks.  scratch: a device buffer of
 * samrs_k_polygon_scratch_bytes(n, h, w, max_edges) bytes; the per-edge outputs of mask j start at entry j * stride with
 * stride = samrs_k_polygon_edge_stride(h, w, max_edges) = min(max_edges, 4 h w); counts_out int32 [n] = edges per mask; a mask
 * with more than max_edges edges has its count and no entries.
 *   samrs_k_polygon_edges  the compact edge list: ids_out uint32 [n][stride] = the edge ids 4 p + d in ascending order, succ_out
 *                          int32 [n][stride] = the compact index of each edge's successor, corner_out uint8 [n][stride] = 1 where
 *                          the edge's direction differs from its predecessor's
 *   samrs_k_polygon_ranks  after the doubling rounds: leader_out int32 [n][stride] = the compact index of the smallest edge of the
 *                          edge's ring, rank_out int32 [n][stride] = the edge's distance from it along the successor */
int64_t samrs_k_polygon_scratch_bytes(int n, int h, int w, int max_edges);
int64_t samrs_k_polygon_edge_stride(int h, int w, int max_edges);
int samrs_k_polygon_edges(const uint8_t* masks, int n, int h, int w, int max_edges, void* scratch, uint32_t* ids_out, int32_t* succ_out,
                          uint8_t* corner_out, int32_t* counts_out, void* stream);
int samrs_k_polygon_ranks(const uint8_t* masks, int n, int h, int w, int max_edges, void* scratch, int32_t* leader_out,
                          int32_t* rank_out, int32_t* counts_out, void* stream);
/* the stages of samrs_simplify_polygons alone (polygon_simplify_kernels.hip).  scratch: a device buffer of
 * samrs_k_polygon_simplify_scratch_bytes(n, vertex_capacity, ring_capacity) bytes (-1: bad arguments), the capacities those of the
 * buffers that samrs_mask_polygons filled.
 *   samrs_k_polygon_simplify_keep  the rows' rings listed, then the rounds: keep_out uint8 [vertex_capacity] = 1 at every kept vertex
 *                                  (absolute index) and 0 elsewhere, kept_out int32 [ring_capacity] = kept vertices of every ring of
 *                                  a placed row (absolute ring index), -1 elsewhere.  Reads vertices, rings and table, changes none. */
int64_t samrs_k_polygon_simplify_scratch_bytes(int n, int64_t vertex_capacity, int64_t ring_capacity);
int samrs_k_polygon_simplify_keep(const int32_t* vertices, const int32_t* rings, const int64_t* table, int n, int eps_q,
                                  int64_t vertex_capacity, int64_t ring_capacity, void* scratch, uint8_t* keep_out, int32_t* kept_out,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SAMRS_HIP_INTERNAL_H */
