// engine_state.h -- private to the engine*.hip files: the state behind a samrs_engine handle, and the helpers that more than one of
// those files uses (namespace samrs_detail).  Whatever one file alone needs stays in that file.
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/samrs_hip.h"
#include "../../include/samrs_hip_internal.h"
#include "common.h"
#include "kernels.h"

namespace samrs_detail {
struct DevTensor {
    float* p = nullptr;           // fp32 on device
    std::vector<int64_t> shape;
    size_t numel = 0;
};

// Per-engine options (samrs_set_option); the environment only supplies the DEFAULTS a new handle starts with:
//   decoder_fusion (SAMRS_DECODER_FUSION, default 1): 0 = run the decoder with its un-fused kernels (separate GEMM / LayerNorm /
//                  product launches) -- the fused-vs-unfused parity test and timing experiments;
//   ln_fold        (SAMRS_LN_FOLD, default 0): fold the encoder blocks' LayerNorms into the qkv / lin1 GEMMs (embed_dim 1280);
//   split          (SAMRS_SPLIT, default 15): bit mask of the rounding points that run as a two-term operand split (3 MFMAs,
//                  ~2^-22 operand error): 1 patch embed, 2 neck, 4 decoder i2t out-projection, 8 decoder upscaler (both
//                  transposed convs).  oracle/error_budget.py measures what each bit buys; DESIGN.md 2 has the table.
//                  16 = the blocks' qkv + proj GEMMs, 32 = the blocks' MLP GEMMs: the REFERENCE-GRADE bits -- three times the MFMA
//                  work of the GEMMs they cover, not part of the default; they need their lo weights, i.e. must be set before
//                  samrs_finalize_weights (SAMRS_SPLIT=63 or the option), and can be cleared / set again afterwards.
// SPLIT_ATTN_V: the attention-side split restricted to the v third of qkv (+ proj): q and k pass through the softmax and buy
// next to nothing (error_budget.py plans4 / plans6); SPLIT_ATTN set as well = all of qkv.  One-launch route only (ViT-H shapes).
// SPLIT_LIN2 (round 4; needs lo_format 4): lin2 alone of the MLP GEMMs takes the lo terms -- the error budget's cheapest way to more margin
// on the multimask outputs (error_budget.py plans10); lin1 then runs on the MX kernel only to have its epilogue emit H's fp4 rows.
enum { SPLIT_PATCH = 1, SPLIT_NECK = 2, SPLIT_OI = 4, SPLIT_UP = 8, SPLIT_DEFAULT = 15, SPLIT_ATTN = 16, SPLIT_MLP = 32, SPLIT_ATTN_V = 64,
       SPLIT_LIN2 = 128, SPLIT_ATTN_ANY = SPLIT_ATTN | SPLIT_ATTN_V, SPLIT_ALL = 255 };

struct DecAttn {
    const float *qw, *qb, *kw, *kb, *vw, *vb, *ow, *ob;
};

struct DecLayer {
    DecAttn self, t2i, i2t;
    const float *n1w, *n1b, *n2w, *n2b, *n3w, *n3b, *n4w, *n4b;
    const float *m1w, *m1b, *m2w, *m2b;
    uint16_t* kvq_w = nullptr;    // ET [384][256] = [Wk_t2i; Wv_t2i; Wq_i2t]
    float* kvq_b = nullptr;       // [384]
    float* kvq_pe = nullptr;      // [tokens][384] = [PE Wk^T | 0 | PE Wq^T]
    uint16_t* i2t_ow = nullptr;   // ET [256][128]
    uint16_t* i2t_ow_lo = nullptr;   // its split remainder
};

// The decoder's fp32 weights outside the transformer layers, resolved once (samrs_finalize_weights), like DecLayer / DecAttn.
struct DecWeights {
    PromptParams prompt{};         // its weight fields; the call fields are filled per call (prompt_call_fields)
    MaskEmbedParams mask_embed{};
    const float* no_mask_embed = nullptr;
    const float *norm_final_w = nullptr, *norm_final_b = nullptr;      // transformer.norm_final_attn
    const float *up_ln_w = nullptr, *up_ln_b = nullptr;                // output_upscaling.1 (LayerNorm2d), for the un-fused upscaler
    const float *head_w[5][3] = {}, *head_b[5][3] = {};                // [0..3] hypernetwork MLPs, [4] the IoU head; 3 layers each
};

struct EncBlock {
    bool global = false;
    const float *ln1w, *ln1b, *ln2w, *ln2b, *qkv_b, *proj_b, *lin1_b, *lin2_b, *rel_h, *rel_w;
    uint16_t *qkv_w = nullptr, *proj_w = nullptr, *lin1_w = nullptr, *lin2_w = nullptr;
    uint16_t *qkv_w_lo = nullptr, *proj_w_lo = nullptr, *lin1_w_lo = nullptr, *lin2_w_lo = nullptr;   // reference-grade bits only
    // copies of qkv_w / lin1_w with a row stride of ldk elements instead of K = D (engine field ldk: operands off the 2560-byte stride)
    uint16_t *qkv_wp = nullptr, *lin1_wp = nullptr;
    // option "lo_format" = 4: the lo terms of the attention-side split on MXFP4 operands (gemm.hip gemm_et_mx_kernel): fp4 codes of
    // hi and lo of the weights + their scale tiles (B layout); proj's K axis padded per head (80 -> 96) so that no MX block
    // straddles two heads
    unsigned char *qkv_w4[2] = {nullptr, nullptr}, *qkv_s4[2] = {nullptr, nullptr};       // [0] = hi, [1] = lo
    unsigned char *proj_w4[2] = {nullptr, nullptr}, *proj_s4[2] = {nullptr, nullptr};
    // ... and of the MLP weights (bit 32): lin1 plain, lin2 on the K axis that lin1's epilogue writes its MX rows on (80 -> 96 per wave tile)
    unsigned char *lin1_w4[2] = {nullptr, nullptr}, *lin1_s4[2] = {nullptr, nullptr};
    unsigned char *lin2_w4[2] = {nullptr, nullptr}, *lin2_s4[2] = {nullptr, nullptr};
    // Outlier columns (option "outlier_cols"; oracle/outlier_budget.py): per block GEMM ([0] qkv, [1] lin1, [2] lin2, [3] proj) the K-columns
    // whose operand magnitude x weight column norm stands out (> ratio x the median), at most 32, picked from the fp32 weights at load
    // time.  For qkv / lin1 their hi + lo split rides as 64 extra K columns of the same launch: the LayerNorm writes the operand side
    // (encoder_kernels.hip), qkv_wx / lin1_wx are dense [N][D + 64] copies of the weights with the weight side appended (on the
    // padded-stride route the same 64 columns sit in the pad region of qkv_wp / lin1_wp instead).
    int oc_n[4] = {0, 0, 0, 0};
    int* oc_idx[4] = {nullptr, nullptr, nullptr, nullptr};
    // share of the picked columns in the GEMM's squared-score mass (sum over S of score^2 / sum over all columns): > 1/2 = the operand error
    // of this GEMM is dominated by its outlier columns.  Decides between the exact f16 lo terms of those columns and the MXFP4 lo terms of
    // ALL columns in the v-third modes (block_route: oc_dominant)
    float oc_share[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t oc_heads = 0;         // bit h: attention head h holds an outlier column of proj (the only heads whose output remainder is needed)
    uint16_t *qkv_wx = nullptr, *lin1_wx = nullptr;
    // lin2 / proj: their A operands (GELU(lin1), the attention output) are written by other kernels, so the 64 columns travel as a
    // dense side operand A_x [M][64] (engine OCX) against oc_bx [D][64] = W_hi[:, S] | W_lo[:, S], one more K stage of the same
    // launch (gemm.hip EXT).  lin2's A_x needs GELU(lin1) of the outlier hidden units BEFORE its rounding: a side GEMM of the
    // LayerNorm output against those <= 32 rows of lin1's weight (lin2_ws, lin2_sb the matching bias) with the exact GELU and the split in
    // its epilogue (encoder_kernels.hip outlier_side_gemm_kernel).
    uint16_t* oc_bx[4] = {nullptr, nullptr, nullptr, nullptr};      // [2] lin2, [3] proj
    uint16_t* lin2_ws = nullptr;       // [32][D (+ 64 when lin1 carries outlier columns of its own)]
    float* lin2_sb = nullptr;          // [32]
    // LayerNorm folded into qkv / lin1 (ViT-H): W diag(gamma) in ET, its row sums, b + W beta
    uint16_t *qkv_wf = nullptr, *lin1_wf = nullptr;
    float *qkv_c = nullptr, *qkv_bf = nullptr, *lin1_c = nullptr, *lin1_bf = nullptr;
};

// a device buffer that an entry point grows on demand and the handle keeps for its next call (scratch_reserve)
struct DeviceScratch { void* p = nullptr; size_t bytes = 0; };
}  // namespace samrs_detail
using namespace samrs_detail;      // this header's only readers are the engine files

struct samrs_engine {
    samrs_config cfg{};
    int device = 0;
    int prec = 0;
    bool finalized = false;
    std::string err;
    std::map<std::string, DevTensor> w;        // fp32 device copies keyed by reference name
    std::vector<void*> owned;                   // everything hipMalloc'ed by the engine

    // derived sizes
    int grid = 64, tokens = 4096, D = 0, C = 256, hd = 0, nwin = 5;
    int T_max = 0;
    bool decoder_fusion = true, ln_fold = false;   // per-engine options: the list above enum SPLIT_*; pass_route for the fold
    int split = SPLIT_DEFAULT;
    int split_ready = SPLIT_DEFAULT;                // bits whose lo weights / workspaces exist (fixed at samrs_finalize_weights)
    int gemm_variant = -1;                          // -1 = the library default (launch_gemm_et's automatic choice)
    int split_depth = 0;                            // reference-grade bits apply to the first N blocks (0 = all)
    bool split_passes = false;                      // reference-grade block GEMMs as three accumulating launches instead of one (A/B)
    int lo_format = 0;                              // 0: lo terms on f16 operands (three-segment f16 GEMM); 4: on MXFP4 operands
    bool mx_ready = false;                          // the fp4 weight copies + activation workspaces exist (fixed at samrs_finalize_weights)
    int mx_gp = 0, mx_kp_proj = 0;                  // proj's padded K axis: heads x mx_gp (head_dim rounded up to 32)
    bool mx_mlp_ready = false;                      // the same for the MLP GEMMs (bit 32 set at samrs_finalize_weights)
    int mx_kp_lin2 = 0;                             // lin2's padded K axis: 4 D / 80 x 96
    unsigned char *H4[2] = {nullptr, nullptr}, *SH4[2] = {nullptr, nullptr};       // GELU(lin1) as fp4 hi / lo, written by lin1's epilogue
    unsigned char *Y4[2] = {nullptr, nullptr}, *SY4[2] = {nullptr, nullptr};       // LN output as fp4 hi / lo + scale tiles (A layout)
    unsigned char *AO4[2] = {nullptr, nullptr}, *SAO4[2] = {nullptr, nullptr};     // attention output likewise (padded K axis)
    bool upscaler_fused = true;                     // one-kernel upscaler (upscaler_fused.hip) instead of ConvT1 GEMM + ConvT2 kernel

    // encoder weights / workspaces
    std::vector<EncBlock> blocks;
    uint16_t *patch_w = nullptr, *neck0_w = nullptr, *neck2_w = nullptr;
    uint16_t *patch_w_lo = nullptr, *neck0_w_lo = nullptr, *neck2_w_lo = nullptr;   // split remainders (common.h split2_pack)
    float* X = nullptr;            // residual stream fp32 [Bi*tokens, D]
    uint16_t* Y = nullptr;         // LN out (ET) [Bi*tokens, D]; folded path: the residual stream itself rounded to ET
    float* STATS = nullptr;        // folded path: per-row (mean, M2) of eight 160-column groups [Bi*tokens][8][2]
    float* ROWSTAT = nullptr;      // folded path: per-row (rstd, -rstd mean) [Bi*tokens][2]
    bool can_fold = false;         // embed_dim == 1280 and the folded weights exist
    uint16_t* QKV = nullptr;       // [Bi*tokens, 3D], token order
    uint16_t* AO = nullptr;        // attention out [Bi*tokens, D]
    uint16_t *Ylo = nullptr, *AOlo = nullptr, *Hlo = nullptr;   // reference-grade split: remainders of Y, AO, H
    float* F32T = nullptr;         // reference-grade split: fp32 result of a three-pass qkv / lin1 product [Bi*tokens, 4D]
    uint16_t* VTG = nullptr;       // V of a global-attention block transposed per head: [Bi][heads][hd][tokens]
    uint16_t* H = nullptr;         // MLP hidden [Bi*tokens, 4D]  (also patch im2col / neck im2col)
    float* N1 = nullptr;           // neck fp32 [Bi*tokens, C]
    uint16_t* N1e = nullptr;       // [Bi*tokens, C]
    float* EMB = nullptr;          // [slots][tokens][C] fp32 (token-major)
    std::vector<char> slot_set;
    // Precision is a property of the EMBEDDING: the "split" mask (and the depth its block-GEMM bits reached) a slot's image was
    // encoded with; -1 = installed by samrs_set_embedding (the caller's numbers, nothing to say about them).  samrs_predict
    // checks it against what the requested outputs need (grade_multimask) instead of trusting whoever touched "split" last.
    std::vector<int> slot_split, slot_depth;
    int grade_multimask = 0;       // block-GEMM bits (any of them) the three multimask tokens need on this model; 0 = none
    bool allow_reduced = false;    // option "allow_reduced": multimask predicts on a slot encoded below that grade are the caller's choice
    // option "range_check" (0 off, 1 count, 2 count and fail): after every producer of an MFMA-operand tensor in the encoder a
    // scan counts the elements sitting at the operand type's saturation value (f16: +-65504, what common.h's saturating
    // conversions write) or beyond into *range_counter (device); read through option "saturated"
    int ln_tail = 0;               // option "ln_tail": 1 = the LayerNorm behind proj / lin2 as a tail of those launches (measured slower: off)
    unsigned int* ln_counters = nullptr;   // per 256-row panel: tiles of the running proj / lin2 launch that have stored (gemm.hip LnTail)
    // option "operand_pad" (default 1): the K = D operands of the plain qkv / lin1 launches -- the LayerNorm output and the weights -- are
    // stored with a row stride of ldk = D + 128 elements where D rows are an even number of 256-byte units (ViT-H: 2560 B -> 2816 B), so
    // that the rows a tile fetches per k-slice spread over all memory channels instead of half of them (GemmOpts::ld)
    int operand_pad_on = 1;
    int ldk = 0;                   // 0: no padded copies exist (other widths)
    // option "outlier_cols" (default 7; SAMRS_OUTLIER_COLS; bit 0: qkv / lin1, bit 1: lin2, bit 2: proj): hi + lo terms for the outlier
    // K-columns of the plain block-GEMM launches (EncBlock::oc_*).  Columns are picked in samrs_finalize_weights (the option must be on by then); later it switches their use.
    // "outlier_ratio_pct" (default 400): a column is an outlier when its score exceeds this percentage of its GEMM's median score.
    // Read-only: "outlier_blocks" (blocks with at least one such column in qkv / lin1), "outlier_columns" (their total over the
    // four block GEMMs).  Weights without outliers (every seeded-normal test model) pick nothing: bit-identical, zero cost.
    int outlier_on = 7 /* bit 0: qkv / lin1, bit 1: lin2, bit 2: proj */, outlier_ratio_pct = 400, outlier_blocks = 0, outlier_columns = 0;
    int outlier_dominant_blocks = 0;   // blocks whose qkv or proj operand error is dominated by outlier columns (EncBlock::oc_share > 1/2)
    float* oc_scratch = nullptr;   // load-time scratch: column / row norms
    uint16_t* OCX = nullptr;       // [M][64]: side operand A_x of the running proj / lin2 launch
    bool oc_resid = false;         // some block has outlier columns in lin2 / proj
    int gelu_fast = -1;            // option "gelu_fast": -1 automatic (on in the 1x-rate modes: no block-GEMM bit in "split"), 0 off, 1 on
    int range_check = 0;
    unsigned long long* range_counter = nullptr;
    unsigned long long range_seen = 0;             // counter value at the end of the last checked encoder pass (mode 2)
    // options "range_profile" (0 off, 1 range profile per site, 2 + column statistics of the block GEMMs' A operands) and "audit_passes"
    // (profile the next N encoder passes in mode 2, then switch off): samrs_hip.h samrs_audit_*.  Sites are fixed at samrs_finalize_weights;
    // the device buffers are allocated by the first pass that needs them (audit_prepare).
    struct AuditSite { std::string name; int columns; size_t col_off; };     // columns: K of the site's column statistics (0 = none)
    std::vector<AuditSite> audit_sites;
    size_t audit_columns = 0;                      // sum of AuditSite::columns
    int range_profile = 0, audit_passes = 0;
    long long* audit_rows = nullptr;               // [n_sites][AUDIT_PROFILE_WORDS]
    double* audit_sumsq = nullptr;                 // [audit_columns], site s at col_off
    uint32_t* audit_maxbits = nullptr;             // likewise
    float* audit_partials = nullptr;               // scratch of one column-statistics launch: [max_images * tokens / AUDIT_ROWS_PER_PARTIAL][4 D]
    std::vector<long long> audit_col_rows;         // per site: rows its column statistics have seen (host side)

    // decoder weights
    std::vector<DecLayer> layers;
    DecAttn fin{};
    DecWeights dec{};
    uint16_t* fin_kv_w = nullptr;  // ET [256][256] = [Wk; Wv]
    float *fin_kv_b = nullptr, *fin_pe = nullptr;
    uint16_t *up1_w = nullptr, *up2_w = nullptr, *up1_w_lo = nullptr, *up2_w_lo = nullptr;
    float *up1_b = nullptr, *up2_b = nullptr, *up_ln = nullptr;   // up_ln = LayerNorm2d gamma[64] | beta[64]
    float* PE = nullptr;           // dense PE [tokens][C]

    // decoder workspaces
    float *TOK0 = nullptr, *Q = nullptr, *TA = nullptr, *TQ = nullptr, *TK = nullptr, *TV = nullptr, *TO = nullptr;
    float *MH = nullptr, *QP = nullptr, *KT = nullptr, *VT = nullptr, *O128 = nullptr, *T2IW = nullptr;
    // Per embedding slot, written when the slot's image is set (prepare_slot_keys) and read-only for every predict on it: the
    // layer-0 image side of the two-way transformer without a mask prompt is the same for every box of an image (keys =
    // embedding + no_mask_embed, their k / v / q projections), so a second predict call / box chunk on the image costs nothing here
    float *K0F = nullptr;          // layer-0 keys fp32 [max_images][tokens][C]
    uint16_t* K0E = nullptr;       // ... in the operand type
    uint16_t* KVQ0 = nullptr;      // their K_t2i | V_t2i | Q_i2t projections [max_images][tokens][3 C / 2]
    // The per-prompt workspaces (the token buffers above included) hold decode_alloc prompts: Bb below.  They are listed once, in
    // decode_buffers(), and allocated / grown by grow_decode_workspaces() only.
    int decode_prompts = 0;        // option "decode_prompts": prompts one decoder chain may hold (samrs_create: max_prompts)
    int decode_alloc = 0;          // prompts the workspaces hold now: the largest decode_prompts so far (they never shrink)
    size_t decode_bytes = 0;       // bytes of the per-prompt workspaces allocated now (option "decode_kbytes")
    float* KF = nullptr;           // per-prompt keys fp32 [Bb*tokens][C]
    uint16_t* KE = nullptr;
    uint16_t* KE_lo = nullptr;     // split remainder of the final keys (operand of the first transposed conv)
    float* DENSE = nullptr;        // mask-prompt dense embedding (allocated on first use)
    int* SLOT_OF = nullptr;        // [Bb] slot of every prompt of a chunk that spans several images (samrs_predict_multi; first use)
    uint16_t* KVQ = nullptr;       // [Bb*tokens][384]
    uint16_t* OI = nullptr;        // [Bb*tokens][128]
    float* U1raw = nullptr;        // [Bb*tokens][256]      U1raw / U1 / U2: the upscaler forms other than ONE_KERNEL; first use
    uint16_t* U1 = nullptr;        // [Bb*tokens][256]
    uint16_t* U2 = nullptr;        // [Bb*tokens*4][128]
    float *HY1 = nullptr, *HY2 = nullptr, *HYPER = nullptr, *IOU = nullptr, *LOW = nullptr;

    // grown on demand (scratch_reserve) and kept for the next call
    DeviceScratch rle_scratch;     // COCO RLE (samrs_rle_encode, samrs_rle_encode_placed)
    DeviceScratch rle_decode_scratch;  // tokens -> counts -> boundaries, bit matrix and counters of samrs_rle_decode
    DeviceScratch region_scratch;  // labels + areas + counters of samrs_clean_masks
    DeviceScratch box_scratch;     // row extents of samrs_mask_boxes
    DeviceScratch poly_scratch;    // edge lists and ranking state of samrs_mask_polygons; the rounds' state and staging copy of samrs_simplify_polygons
    // the buffers samrs_mask_polygons traced into, newest last (16 at most): their capacities bound samrs_simplify_polygons's scratch
    struct PolyBuffers { const void* vertices; const void* rings; long long vcap, rcap; };
    std::vector<PolyBuffers> poly_seen;
    DeviceScratch png_scratch;     // class-map PNG scratch (samrs_png_encode_labels)
    DeviceScratch png_rgb_scratch; // filtered bytes + code tables of samrs_png_encode_rgb
    DeviceScratch overlap_scratch; // entry areas of samrs_resolve_overlaps (rule SMALLEST without before_out)
    DeviceScratch ap_scratch;      // matched flags (+ host scores staged) of samrs_coco_match / samrs_coco_match_min
    DeviceScratch boundary_scratch;    // the row-eroded planes of samrs_mask_boundary_bits

    // optional in-situ timing of the dominant kernel (MLP lin1 + GELU GEMM) with HIP events
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tev;   // recorded pairs
    std::vector<hipEvent_t> tpool;                         // recycled events
};

namespace samrs_detail {
inline int fail(samrs_engine* e, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (e) e->err = buf;
    return code;
}

#define CK(e, expr)                                                                                    \
    do {                                                                                               \
        hipError_t _err = (expr);                                                                      \
        if (_err != hipSuccess)                                                                        \
            return fail((e), SAMRS_ERR_HIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_err)); \
    } while (0)

// the kernel-level entry points (no engine to carry the text)
#define KRET(expr)                                                                                  \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) fprintf(stderr, "libsamrs_hip: %s: %s\n", __func__, hipGetErrorString(_e)); \
        return _e == hipSuccess ? SAMRS_OK : SAMRS_ERR_HIP;                                         \
    } while (0)

template <typename T>
hipError_t dalloc(samrs_engine* e, T** p, size_t count) {
    void* q = nullptr;
    hipError_t r = hipMalloc(&q, count * sizeof(T) > 0 ? count * sizeof(T) : 16);
    if (r != hipSuccess) return r;
    e->owned.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return hipSuccess;
}

// Every entry point that touches the device runs on the engine's device and then puts the CALLER's current device
// back (a process that drives several GPUs, or a handle collected at an arbitrary time, must not find its thread's
// device changed under it).
struct DeviceGuard {
    int prev = -1;
    hipError_t status = hipSuccess;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) status = hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
// an engine's own GEMM tile choice (samrs_set_option "gemm_variant") applies to the launches of its entry points only
struct GemmVariantScope {
    int prev;
    explicit GemmVariantScope(int v) : prev(swap_gemm_variant_override(v)) {}
    ~GemmVariantScope() { (void)swap_gemm_variant_override(prev); }
};
#define ON_DEVICE(e) DeviceGuard _dg((e)->device); CK((e), _dg.status); GemmVariantScope _gvs((e)->gemm_variant)

inline const float* W(samrs_engine* e, const std::string& n) { return e->w.at(n).p; }

// the call fields of a PromptParams; its weight fields are the caller's (DecWeights::prompt, or the kernel hook's arguments)
inline void prompt_call_fields(PromptParams& pp, const float* boxes, const float* point_coords, const int32_t* point_labels, int n_prompts,
                               int n_points, float img_size) {
    pp.boxes = boxes; pp.point_coords = point_coords; pp.point_labels = point_labels;
    pp.n_prompts = n_prompts; pp.n_points = point_coords ? n_points : 0;
    pp.img_size = img_size;
}

// tokens per prompt: IoU token + 4 mask tokens, the points (+ the pad point when there is no box), two box corners
inline int point_token_count(bool boxes, int n_points) { return n_points ? n_points + (boxes ? 0 : 1) : 0; }
inline int prompt_token_count(bool boxes, int n_points) { return 5 + point_token_count(boxes, n_points) + (boxes ? 2 : 0); }

// at least `need` bytes afterwards; a smaller buffer is released only after `s` has drained (hipFree then synchronises the device).
// A buffer that already fits costs no HIP call; a failed allocation leaves `sc` empty
hipError_t scratch_reserve(DeviceScratch& sc, size_t need, hipStream_t s);
void scratch_release(DeviceScratch& sc);

// defined in engine.hip (a lazy per-prompt decoder workspace) and engine_encode.hip (the checkpoint audit)
int need_decode_buffer(samrs_engine* e, const char* name);
void audit_build_sites(samrs_engine* e);
int audit_reset(samrs_engine* e);
}  // namespace samrs_detail
