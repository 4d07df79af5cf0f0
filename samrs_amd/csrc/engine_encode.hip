// engine_encode.hip -- the encoder pass (samrs_set_images and its siblings): its routes and run_* steps, the checkpoint audit that
// rides on it (samrs_audit_*), and the embedding store with the slots' layer-0 decoder keys.
// The launch sequence follows the reference graph (paths under Generate Dataset/segment_anything/), restated for this kernel set:
//   set_images : modeling/sam.py:164-174 -> modeling/image_encoder.py:106-116,166-182,88-104
#include "engine_state.h"

// ---- checkpoint audit (options "range_profile" / "audit_passes") --------------------------------------------------------------------
enum { AUDIT_QKV_IN = 0, AUDIT_Q, AUDIT_K, AUDIT_V, AUDIT_PROJ_IN, AUDIT_LIN1_IN, AUDIT_LIN2_IN, AUDIT_PER_BLOCK };
enum { AUDIT_NECK1_IN = 0, AUDIT_NECK2_IN, AUDIT_KEYS0, AUDIT_TAIL };

namespace samrs_detail {
void audit_build_sites(samrs_engine_t* e) {
    static const char* const per_block[AUDIT_PER_BLOCK] = {"qkv_in", "q", "k", "v", "proj_in", "lin1_in", "lin2_in"};
    e->audit_sites.clear();
    e->audit_columns = 0;
    auto add = [&](const std::string& name, int columns) {
        e->audit_sites.push_back({name, columns, e->audit_columns});
        e->audit_columns += (size_t)columns;
    };
    for (int i = 0; i < e->cfg.depth; ++i)
        for (int k = 0; k < AUDIT_PER_BLOCK; ++k)
            add("blocks." + std::to_string(i) + "." + per_block[k],
                (k == AUDIT_QKV_IN || k == AUDIT_PROJ_IN || k == AUDIT_LIN1_IN) ? e->D : k == AUDIT_LIN2_IN ? 4 * e->D : 0);
    add("neck.conv1_in", 0); add("neck.conv2_in", 0); add("decoder.keys0", 0);
    e->audit_col_rows.assign(e->audit_sites.size(), 0);
}

// forget everything profiled so far (device-synchronising: a pass may still be adding to the buffers)
int audit_reset(samrs_engine_t* e) {
    if (e->audit_rows || e->audit_sumsq) CK(e, hipDeviceSynchronize());
    if (e->audit_rows) CK(e, hipMemset(e->audit_rows, 0, e->audit_sites.size() * AUDIT_PROFILE_WORDS * sizeof(long long)));
    if (e->audit_sumsq) {
        CK(e, hipMemset(e->audit_sumsq, 0, e->audit_columns * sizeof(double)));
        CK(e, hipMemset(e->audit_maxbits, 0, e->audit_columns * sizeof(uint32_t)));
    }
    e->audit_col_rows.assign(e->audit_sites.size(), 0);
    return SAMRS_OK;
}
}  // namespace samrs_detail

// the device buffers, zeroed, on first use (the caller is on the engine's device)
static int audit_prepare(samrs_engine_t* e, bool with_columns) {
    if (!e->audit_rows) {
        const size_t n = e->audit_sites.size() * AUDIT_PROFILE_WORDS;
        CK(e, dalloc(e, &e->audit_rows, n));
        CK(e, hipMemset(e->audit_rows, 0, n * sizeof(long long)));
        CK(e, hipDeviceSynchronize());
    }
    if (with_columns && !e->audit_sumsq) {
        CK(e, dalloc(e, &e->audit_sumsq, e->audit_columns));
        CK(e, dalloc(e, &e->audit_maxbits, e->audit_columns));
        CK(e, dalloc(e, &e->audit_partials, column_stats_partial_floats(e->cfg.max_images * e->tokens, 4 * e->D)));
        CK(e, hipMemset(e->audit_sumsq, 0, e->audit_columns * sizeof(double)));
        CK(e, hipMemset(e->audit_maxbits, 0, e->audit_columns * sizeof(uint32_t)));
        CK(e, hipDeviceSynchronize());          // the zeros are in place before a pass on another stream adds to them
    }
    return SAMRS_OK;
}

// option "range_profile": one site of the running pass: `rows` rows of `cols` live elements at a stride of `ld`, right behind the tensor's
// producer on `s`.  The sites are the places the range check scans (q | k | v apart; the D live columns of a LayerNorm output only, not
// its outlier extension, whose hi half is a copy)
static int audit_site(samrs_engine_t* e, int site, const uint16_t* x, int rows, int cols, int ld, hipStream_t s) {
    if (!e->range_profile) return SAMRS_OK;
    if (site < 0 || site >= (int)e->audit_sites.size()) return fail(e, SAMRS_ERR_BAD_ARG, "audit site %d out of range", site);
    CK(e, launch_range_profile(e->prec, x, (long)rows * cols, cols, ld, e->audit_rows + (size_t)site * AUDIT_PROFILE_WORDS, s));
    const samrs_engine::AuditSite& a = e->audit_sites[site];
    if (e->range_profile == 2 && a.columns == cols) {
        CK(e, launch_column_stats(e->prec, x, rows, cols, ld, e->audit_partials, e->audit_sumsq + a.col_off, e->audit_maxbits + a.col_off, s));
        e->audit_col_rows[site] += rows;
    }
    return SAMRS_OK;
}

// option "range_check": scan an operand tensor (`count` elements) right after its producer (same stream).  cols / ld: a tensor whose rows
// carry pad columns (the LayerNorm output on the padded-stride route): the `cols` live columns of rows at a stride of `ld` only
static int range_scan(samrs_engine_t* e, const void* x, size_t count, hipStream_t s, int cols = 0, int ld = 0) {
    if (e->range_check) CK(e, launch_range_scan(e->prec, x, (long)count, e->range_counter, s, cols, ld));
    return SAMRS_OK;
}

// X (the fp32 residual stream) += A W^T + A_x B_x^T + bias -- proj / lin2 with the hi + lo terms of their outlier columns (EncBlock::oc_bx):
// one launch with one more K stage where the 256 x 320 pair-stage kernel takes the shape (gemm.hip EXT), else the plain launch followed
// by an accumulating launch of the 64-column side product on the 128 x 128 kernel (any shape; small models only: it re-reads X)
static hipError_t resid_gemm_ext(samrs_engine* e, int prec, const void* A, const void* Wt, const void* Ax, const void* Bx, const float* bias,
                                 int M, int N, int K, hipStream_t s) {
    if (gemm_ext_ok(M, N, K)) return launch_gemm_et_ext(prec, A, Wt, Ax, Bx, e->X, bias, M, N, K, s);
    const hipError_t r = launch_gemm_et(prec, A, Wt, e->X, bias, nullptr, 0, M, N, K, true, false, true, s);
    if (r != hipSuccess) return r;
    GemmVariantScope base_kernel(1);
    return launch_gemm_et(prec, Ax, Bx, e->X, nullptr, nullptr, 0, M, N, 64, true, false, true, s);
}

// C (fp32 [M][N]) (+)= A B^T + A_lo B^T + A B_lo^T + bias (+ add2d): the product of hi + lo operands (common.h split2_pack) without
// its lo x lo term.  ONE launch over a three-segment K axis where the caller found the shape to fit the pair-stage tile
// (`one_launch`: gemm_split3_ok; gemm.hip seg_src_a), else three accumulating passes.  fp32 accumulation order is part of the result, so
// the three passes keep the order of their site: FIRST = hi x hi (with the bias and the addend), lo x B, A x B_lo -- patch embed and
// the neck; LAST = lo x B, A x B_lo, then hi x hi with the bias -- the block GEMMs.  `accumulate`: C already holds a value to add to
// (the residual stream under proj / lin2).
enum class MainPass { FIRST, LAST };
static hipError_t gemm_hilo(int prec, bool one_launch, MainPass order, const void* A, const void* A_lo, const void* B, const void* B_lo,
                            float* C, const float* bias, const float* add2d, int add2d_period, int M, int N, int K, bool accumulate,
                            hipStream_t s) {
    if (one_launch) return launch_gemm_et_split3(prec, A, A_lo, B, B_lo, C, bias, M, N, K, true, accumulate, s, 0, add2d, add2d_period);
    hipError_t r = hipSuccess;
    if (order == MainPass::FIRST) r = launch_gemm_et(prec, A, B, C, bias, add2d, add2d_period, M, N, K, true, false, accumulate, s);
    if (r == hipSuccess) r = launch_gemm_et(prec, A_lo, B, C, nullptr, nullptr, 0, M, N, K, true, false, accumulate || order == MainPass::FIRST, s);
    if (r == hipSuccess) r = launch_gemm_et(prec, A, B_lo, C, nullptr, nullptr, 0, M, N, K, true, false, true, s);
    if (r == hipSuccess && order == MainPass::LAST) r = launch_gemm_et(prec, A, B, C, bias, add2d, add2d_period, M, N, K, true, false, true, s);
    return r;
}

// ---- the encoder pass: which launches it takes, decided before anything is launched ------------------------------------------------
// pass_route / block_route read engine fields and the gemm_*_ok predicates only: they launch nothing, allocate nothing and touch no
// device memory.  run_patch_embed / run_block_* / run_neck below do what the routes say and decide nothing.
namespace {
// What holds for every block of one encode() call: from the engine's options and readiness flags, M and n_blocks.
struct PassRoute {
    int M = 0;                     // rows of the pass: tiles x tokens
    int n_blocks = 0;              // blocks the pass runs (samrs_debug_encoder_prefix stops early)
    bool sp_patch = false, sp_neck = false;     // patch embed / both neck convolutions on hi + lo operands
    bool one3 = false;             // a hi + lo product as ONE launch where its shape fits (else, and under "split_passes", three passes)
    bool fold = false;             // LayerNorms folded into the qkv / lin1 GEMMs
    int depth_full = 0, depth_v = 0;            // blocks the full block-GEMM bits (16 / 32 / 128) / the v-third form (64) reach
    bool fast_gelu = false;        // the cheaper erf in the plain lin1 launch's GELU epilogue
    bool ln_tail = false;          // norm2 / the next norm1 as a tail of the proj / lin2 launches
    bool pad_ok = false;           // the plain qkv / lin1 launches may read the padded-stride operands
    bool oc_any = false, oc_ok = false;         // outlier columns in use at all / in the plain qkv + lin1 launches (bit 0)
};

static PassRoute pass_route(const samrs_engine_t* e, int M, int n_blocks) {
    const samrs_config& c = e->cfg;
    const int D = e->D;
    PassRoute p;
    p.M = M;
    p.n_blocks = n_blocks;
    // SPLIT_PATCH: pixels and weights as hi + lo (three GEMM passes into X) -- the normalised pixel values span +-2.6 and
    // their f16 rounding alone cost 266 of the 899 class-map pixels the round-2 engine lost at ViT-H (oracle/error_budget.py)
    p.sp_patch = (e->split & SPLIT_PATCH) != 0;
    // SPLIT_NECK: both neck convolutions on hi + lo operands (three GEMM passes each; 0.13 % of the encoder FLOPs).  The neck is
    // the last thing in front of the embedding: nothing downstream averages its operand rounding away (error_budget.py:
    // 258 + 259 of 899 class-map pixels at ViT-H).
    p.sp_neck = (e->split & SPLIT_NECK) != 0;
    // LayerNorm folding (encoder blocks, embed_dim 1280 only).  OFF by default: measured slower than the stand-alone LayerNorm
    // kernel on MI355X (anything added to a GEMM epilogue runs while the matrix pipe idles, the stand-alone kernel
    // streams at ~6 TB/s).  SAMRS_LN_FOLD=1 at load time or samrs_set_option(e, "ln_fold", 1) BEFORE samrs_finalize_weights prepares
    // the folded weights; the switch can then be flipped at run time (A/B runs, the folded-vs-unfolded parity test).
    // Folded LayerNorm: no LayerNorm launches inside the blocks.  Y holds the residual stream rounded to ET and
    // STATS its per-row partial statistics, both written by the epilogue of the GEMM that produced X (proj, lin2; in front of block 0,
    // once, by rowstats_convert); qkv / lin1 run on the gamma-folded weights and normalise in their epilogue (gemm.hip).
    // reference-grade bits: the block GEMMs on hi + lo operands (qkv / lin1: three passes into an fp32 scratch, then one
    // rounding to the operand type; proj / lin2: two more accumulating passes into the residual stream) -- never with the fold
    p.fold = e->can_fold && e->ln_fold && !(e->split & SPLIT_ATTN_ANY) && !(e->split & SPLIT_MLP);
    // "split_depth" > 0: the block-GEMM bits apply to the first split_depth blocks only -- an operand error made early is carried
    // (and amplified) through every later block, one made in the last blocks is not (error_budget.py plans5 / plans6)
    // 0 = automatic: every block for the full bits (16 / 32), the leading three quarters for the v-third form (64)
    p.depth_full = e->split_depth > 0 ? e->split_depth : c.depth;
    p.depth_v = e->split_depth > 0 ? e->split_depth : (3 * c.depth + 3) / 4;
    // the three split terms of a block GEMM as ONE launch over a three-segment K axis (gemm.hip seg_src_a) where the shape
    // fits the 256 x 320 tile (ViT-H); SAMRS_SPLIT_PASSES=1 / option "split_passes" keeps the three accumulating launches (A/B).
    // Patch embed and the neck likewise, where their shapes fit the pair-stage tile.
    p.one3 = !e->split_passes;
    // the 1x-rate modes take the cheaper erf in lin1's GELU epilogue (common.h gelu_erf2_et: -3.3 % on the dominant kernel);
    // every mode with a block-GEMM split bit keeps the arithmetic its parity statistics were measured on, bit for bit
    p.fast_gelu = e->gelu_fast >= 0 ? e->gelu_fast != 0 : !(e->split & (SPLIT_ATTN_ANY | SPLIT_MLP | SPLIT_LIN2));
    // The LayerNorm behind proj (norm2) and behind lin2 (the next block's norm1) as a tail of those GEMMs (gemm.hip LnTail): OPT-IN
    // (option "ln_tail" = 1).  Built, bit-identical with the stand-alone kernel, and measured slower (profiles/r05_ln_tail.txt): the
    // panel is normalised by ONE CU, and one CU draws ~20 GB/s from HBM -- 62 us for the 1.3 MB of a panel, against 53 us for a
    // LayerNorm launch that uses all 256.  The 1x-rate modes only (the reference-grade modes want the LayerNorm's lo / MXFP4 outputs),
    // and only where the shapes take the 256 x 320 kernel (at least one full round of tiles: batches of 4 tiles and more at ViT-H).
    p.ln_tail = !p.fold && !(e->split & (SPLIT_ATTN_ANY | SPLIT_MLP | SPLIT_LIN2)) && e->ln_tail > 0 &&
                e->ln_counters && gemm_lntail_ok(M, D, D) && gemm_lntail_ok(M, D, 4 * D);
    // padded operand rows for the plain qkv / lin1 launches (they run on the persistent ET kernels at these shapes: gemm_ld_ok)
    p.pad_ok = e->ldk && e->operand_pad_on && !p.fold && !p.ln_tail;
    // outlier-column extension of the plain qkv / lin1 launches (EncBlock::oc_*): not with the folded / tail LayerNorm forms (other producers of Y)
    p.oc_any = e->outlier_on && e->outlier_columns > 0 && !p.fold && !p.ln_tail;
    p.oc_ok = p.oc_any && (e->outlier_on & 1);
    return p;
}

// The form a block's LayerNorm runs in.  NONE: no launch (folded into the GEMM behind it).  TAIL: no launch either, the GEMM in front of
// it wrote Y (gemm.hip LnTail).  LO: also writes the remainder Ylo.  MX: also writes the fp4 codes + scales of hi and lo (Y4 / SY4).
enum class Norm { NONE, TAIL, PLAIN, LO, MX };
// The form a block GEMM runs in.  FOLD: the gamma-folded weights (qkv / lin1) or the statistics epilogue (proj / lin2).  MX: lo terms on
// MXFP4 operands in the same launch.  SPLIT3: the hi + lo product on f16 operands, one launch or three passes (gemm_hilo; *_one).
// PLAIN: hi x hi alone.  LNTAIL (proj / lin2): plain with the following LayerNorm as its tail.  EXT (proj / lin2): plain plus the
// hi + lo terms of the outlier columns as one more K stage (resid_gemm_ext).
enum class Gemm { FOLD, MX, SPLIT3, PLAIN, LNTAIL, EXT };
// which copy of the qkv / lin1 weights a launch reads: dense rows of K = D, rows at the padded stride ldk (the outlier extension in their
// pad region), dense rows of D + 64 with the outlier extension appended
enum class Wcopy { W, WP, WX };

// The launches of one block, from the pass route, the EncBlock and its index.
struct BlockRoute {
    Norm norm1 = Norm::PLAIN, norm2 = Norm::PLAIN;
    Gemm qkv = Gemm::PLAIN, proj = Gemm::PLAIN, lin1 = Gemm::PLAIN, lin2 = Gemm::PLAIN;
    bool qkv_one = false, proj_one = false, lin1_one = false, lin2_one = false;     // SPLIT3: one launch (else three passes)
    // norm1 + qkv
    int v_from = 0;                // qkv SPLIT3 (one launch) / MX: the first output column that takes the lo terms (2 D = the v third alone)
    int noc = 0;                   // outlier columns of norm1's output riding in the qkv launch (64 more K columns)
    Wcopy qkv_wc = Wcopy::W;
    int qkv_K = 0, qkv_ld = 0;     // K of the qkv launch; operand row stride it reads A and B with (0 = K)
    int norm1_ld = 0;              // row stride norm1 writes Y with (0 = D)
    int y1_ld = 0, y1_live = 0;    // after norm1: row stride Y holds, and how many columns of a row are operand values (the scans)
    // attention
    bool mx_ao = false;            // the attention kernels write the proj GEMM's MX operands themselves
    bool ao_lo = false;            // ... and the lo half of their output (AOlo)
    int nop = 0;                   // outlier columns of proj (EXT)
    uint32_t lo_heads = 0xffffffffu;            // windowed attention: the heads whose output remainder is needed
    // norm2 + lin1
    int nol = 0;                   // outlier columns of norm2's output riding in the lin1 launch
    Wcopy lin1_wc = Wcopy::W;
    int lin1_K = 0, lin1_ld = 0;
    int norm2_ld = 0;
    int y2_ld = 0, y2_live = 0;    // after norm2, as y1_*
    int lin1_mx_from = 0;          // lin1 MX: first output column with lo terms (N = none: the launch only emits H's MX rows)
    // lin2
    int nol2 = 0;                  // outlier columns of lin2 (EXT)
    int side_ld = 0;               // ... row stride of the LayerNorm output their side GEMM reads back from Y
    bool next_rowstat = false;     // FOLD: row statistics for the next block's qkv
};

static BlockRoute block_route(const samrs_engine_t* e, const PassRoute& p, const EncBlock& b, int i) {
    const int D = e->D, M = p.M, depth = e->cfg.depth;
    BlockRoute r;
    const bool attn_full = (e->split & SPLIT_ATTN) && i < p.depth_full;
    // v-third modes (79 / 207): where the outlier columns carry more than half of this block's qkv or proj operand-error mass, the block
    // runs the plain launches with the EXACT f16 lo terms of those columns instead of the MXFP4 lo terms of all columns -- an outlier
    // column shares its fp4 block scale with 31 neighbours (their lo terms quantise to zero, its own keeps ~2 bits).  Measured on
    // heavy-tailed weights (tests/test_outlier_gpu.py): multimask IoU min 0.99848 -> the 1x-rate mode's 0.99906 with the columns treated.
    const bool oc_dominant = p.oc_any && (e->outlier_on & 5) == 5 && !attn_full && (b.oc_share[0] > 0.5f || b.oc_share[3] > 0.5f);
    const bool sp_attn = attn_full || ((e->split & SPLIT_ATTN_V) && i < p.depth_v && !oc_dominant);
    const bool sp_mlp = (e->split & SPLIT_MLP) && i < p.depth_full;
    const bool mx_mlp = e->lo_format == 4 && e->mx_mlp_ready && !e->split_passes && gemm_mx_ok(M, 4 * D, D, D) && gemm_mx_ok(M, D, 4 * D, e->mx_kp_lin2);
    const bool sp_lin2 = (e->split & SPLIT_LIN2) && !sp_mlp && mx_mlp && i < p.depth_full;     // lin2 alone (lin1 only emits H's MX rows)
    const bool mx_attn = e->lo_format == 4 && e->mx_ready && !e->split_passes && gemm_mx_ok(M, 3 * D, D, D) && (2 * D) % 320 == 0;

    // norm1 + qkv in plain token order for both block kinds; the windowed kernel partitions
    // on the fly and takes k / v of padding positions from the qkv bias
    r.qkv_K = D; r.y1_ld = D; r.y1_live = D;
    if (p.fold) {
        r.norm1 = Norm::NONE; r.qkv = Gemm::FOLD;
    } else if (sp_attn && mx_attn) {
        // lo terms on MXFP4 operands: the LayerNorm emits the fp4 codes + scales of its output's hi and lo (no ET lo copy).
        // Outlier columns of norm1's output: the v third is covered by its fp4 correction segments (they span every column); the q and k
        // tiles of the v-third form run plain f16 and read the 64-column extension of the padded rows as one more stage
        r.norm1 = Norm::MX; r.qkv = Gemm::MX;
        r.v_from = attn_full ? 0 : 2 * D;
        r.noc = (p.oc_ok && !attn_full && b.oc_n[0] && e->ldk && b.qkv_wp) ? b.oc_n[0] : 0;
        if (r.noc) { r.qkv_wc = Wcopy::WP; r.qkv_ld = r.norm1_ld = r.y1_ld = e->ldk; r.y1_live = D + 64; }
    } else if (sp_attn) {
        r.norm1 = Norm::LO; r.qkv = Gemm::SPLIT3;
        r.qkv_one = p.one3 && gemm_split3_ok(M, 3 * D, D);     // one launch, ET output rounded once from the register accumulators
        // v third only: needs the tile mask of the one-launch kernel; other shapes split all of qkv
        r.v_from = (!attn_full && r.qkv_one && (2 * D) % 320 == 0) ? 2 * D : 0;
    } else {
        // outlier columns of norm1's output: 64 more K columns (lo | hi of up to 32 columns) in the same launch -- on the padded-stride
        // route in the pad region of the rows (K = D + 64 of the ldk-element rows), elsewhere on dense rows of D + 64 elements
        r.noc = (p.oc_ok && b.oc_n[0] && b.qkv_wx) ? b.oc_n[0] : 0;
        r.qkv_K = r.noc ? D + 64 : D;
        r.qkv_ld = (p.pad_ok && b.qkv_wp && gemm_ld_ok(M, 3 * D, r.qkv_K, false)) ? e->ldk : 0;
        r.qkv_wc = r.qkv_ld ? Wcopy::WP : (r.noc ? Wcopy::WX : Wcopy::W);
        r.y1_ld = r.qkv_ld ? r.qkv_ld : r.qkv_K;                // row stride of Y for this launch
        r.y1_live = r.qkv_K;
        r.norm1_ld = r.y1_ld == D ? 0 : r.y1_ld;
    }

    // attention
    r.mx_ao = sp_attn && mx_attn;
    // outlier columns of proj (plain launch only): the attention kernel also writes the lo half of its output, a gather makes A_x
    r.nop = (p.oc_any && (e->outlier_on & 4) && !sp_attn && b.oc_n[3] && b.oc_bx[3] && e->AOlo && e->OCX) ? b.oc_n[3] : 0;
    r.ao_lo = (sp_attn && !r.mx_ao) || r.nop;
    // the remainder only feeds the gather of proj's outlier columns: the heads that hold them
    r.lo_heads = r.nop ? b.oc_heads : 0xffffffffu;

    // proj (adds into the residual stream)
    if (p.fold) r.proj = Gemm::FOLD;
    // the attention kernel wrote hi / lo of its output as fp4 on the per-head padded K axis
    else if (sp_attn && mx_attn) r.proj = Gemm::MX;
    else if (sp_attn) { r.proj = Gemm::SPLIT3; r.proj_one = p.one3 && gemm_split3_ok(M, D, D); }
    else if (p.ln_tail) r.proj = Gemm::LNTAIL;
    else if (r.nop) r.proj = Gemm::EXT;

    // norm2 + lin1.  lin1 takes the plain launch exactly when none of these holds; then norm2 writes the padded layout for it
    const bool lin1_plain = !p.fold && !sp_lin2 && !sp_mlp;
    r.nol = (p.oc_ok && lin1_plain && b.oc_n[1] && b.lin1_wx) ? b.oc_n[1] : 0;    // outlier columns of norm2's output (see qkv above)
    r.lin1_K = r.nol ? D + 64 : D;
    r.lin1_ld = (p.pad_ok && b.lin1_wp && lin1_plain && gemm_ld_ok(M, 4 * D, r.lin1_K, true)) ? e->ldk : 0;
    r.lin1_wc = r.lin1_ld ? Wcopy::WP : (r.nol ? Wcopy::WX : Wcopy::W);
    r.side_ld = r.lin1_ld ? r.lin1_ld : r.lin1_K;
    r.y2_ld = D; r.y2_live = D;
    if (p.fold) r.norm2 = Norm::NONE;
    else if (r.proj == Gemm::LNTAIL) r.norm2 = Norm::TAIL;         // norm2 came out of the proj launch
    else if (sp_mlp && mx_mlp) r.norm2 = Norm::MX;
    else {
        r.norm2 = sp_mlp ? Norm::LO : Norm::PLAIN;
        r.norm2_ld = (sp_mlp || r.side_ld == D) ? 0 : r.side_ld;
        if (r.norm2_ld) { r.y2_ld = r.norm2_ld; r.y2_live = r.lin1_K; }
    }
    if (p.fold) r.lin1 = Gemm::FOLD;
    // lin1 without lo terms (split_from_n = N: no MX stages; the a4 / b4 operands are not touched), its epilogue emits H's fp4 rows
    else if (sp_lin2) { r.lin1 = Gemm::MX; r.lin1_mx_from = 4 * D; }
    // lo terms on MXFP4: ET output with the exact-erf GELU in the epilogue, which also emits H as fp4 hi / lo for lin2
    else if (sp_mlp && mx_mlp) r.lin1 = Gemm::MX;
    else if (sp_mlp) { r.lin1 = Gemm::SPLIT3; r.lin1_one = p.one3 && gemm_split3_ok(M, 4 * D, D); }

    // lin2 (adds into the residual stream)
    // outlier columns of lin2 (plain launches only): the pre-activations of those <= 32 hidden units once more, in fp32, from the
    // LayerNorm output that still sits in Y (rows of stride side_ld) -> exact GELU -> lo | hi = A_x
    r.nol2 = (p.oc_any && (e->outlier_on & 2) && lin1_plain && b.oc_n[2] && b.oc_bx[2] && e->OCX && b.lin2_ws &&
              // the side weights carry lin1's own extension columns: Y must hold them in this launch (else they are stale)
              (b.oc_n[1] == 0 || r.nol > 0)) ? b.oc_n[2] : 0;
    if (p.fold) { r.lin2 = Gemm::FOLD; r.next_rowstat = i + 1 < depth; }
    else if ((sp_mlp && mx_mlp) || sp_lin2) r.lin2 = Gemm::MX;
    else if (sp_mlp) { r.lin2 = Gemm::SPLIT3; r.lin2_one = p.one3 && gemm_split3_ok(M, D, 4 * D); }
    // the next block's norm1 comes out of this launch: that block then starts with Y ready (run_block_attn: y_ready)
    else if (p.ln_tail && i + 1 < depth && i + 1 < p.n_blocks) r.lin2 = Gemm::LNTAIL;
    else if (r.nol2) r.lin2 = Gemm::EXT;
    return r;
}

static const uint16_t* weight_copy(Wcopy c, const uint16_t* w, const uint16_t* wp, const uint16_t* wx) {
    return c == Wcopy::WP ? wp : c == Wcopy::WX ? wx : w;
}

// a block's LayerNorm of the residual stream into Y, in the form its route names (NONE / TAIL: nothing to launch)
static hipError_t run_norm(samrs_engine_t* e, Norm form, const float* gamma, const float* beta, int M, int ld, const int* oc_idx, int n_oc,
                           hipStream_t s) {
    if (form == Norm::NONE || form == Norm::TAIL) return hipSuccess;
    const bool mx = form == Norm::MX;
    return launch_layernorm(e->prec, e->X, gamma, beta, 1e-6f, e->Y, nullptr, M, e->D, 0, e->grid, 0, s, form == Norm::LO ? e->Ylo : nullptr,
                            mx ? e->Y4[0] : nullptr, mx ? e->Y4[1] : nullptr, mx ? e->SY4[0] : nullptr, mx ? e->SY4[1] : nullptr, ld,
                            n_oc ? oc_idx : nullptr, n_oc);
}
}  // namespace

// patch embed: im2col (normalise + zero pad) -> GEMM (+bias +pos_embed) -> X.  One im2col launch per run of
// same-size tiles that sit back to back in memory (the whole batch for a contiguous tile stack).
static int run_patch_embed(samrs_engine_t* e, const PassRoute& p, const uint8_t* const* images, const int* in_h, const int* in_w, int n,
                           hipStream_t s) {
    const samrs_config& c = e->cfg;
    const int D = e->D, tokens = e->tokens, prec = e->prec, M = p.M;
    const size_t KP = (size_t)3 * c.patch_size * c.patch_size;
    uint16_t* Hlo = e->H + (size_t)M * KP;
    for (int i = 0; i < n;) {
        int j = i + 1;
        while (j < n && in_h[j] == in_h[i] && in_w[j] == in_w[i] &&
               images[j] == images[i] + (size_t)(j - i) * in_h[i] * in_w[i] * 3) ++j;
        CK(e, launch_patch_im2col(prec, images[i], e->H + (size_t)i * tokens * KP, j - i, in_h[i], in_w[i], e->grid, c.patch_size, s,
                                  p.sp_patch ? Hlo + (size_t)i * tokens * KP : nullptr));
        i = j;
    }
    const float *bias = W(e, "image_encoder.patch_embed.proj.bias"), *pos = W(e, "image_encoder.pos_embed");
    if (p.sp_patch)
        CK(e, gemm_hilo(prec, p.one3 && gemm_split3_ok(M, D, (int)KP, true), MainPass::FIRST, e->H, Hlo, e->patch_w, e->patch_w_lo, e->X,
                        bias, pos, tokens, M, D, (int)KP, false, s));
    else
        CK(e, launch_gemm_et(prec, e->H, e->patch_w, e->X, bias, pos, tokens, M, D, (int)KP, true, false, false, s));
    if (p.fold && p.n_blocks > 0) {        // the folded blocks' first operands: ET(X) and its row statistics
        CK(e, launch_rowstats_convert(prec, e->X, e->Y, e->STATS, M, D, s));
        CK(e, launch_ln_rowstat(e->STATS, e->ROWSTAT, M, 1e-6f, s));
    }
    return SAMRS_OK;
}

// First half of block i: norm1 -> qkv -> attention (+ the scans of their operands) -> proj -> norm2.
// y_ready: Y already holds norm1 of this block (written by the previous block's lin2 launch, run_block_mlp)
static int run_block_attn(samrs_engine_t* e, const PassRoute& p, const BlockRoute& r, const EncBlock& b, int i, int n, bool y_ready,
                          hipStream_t s) {
    const samrs_config& c = e->cfg;
    const int D = e->D, g = e->grid, prec = e->prec, M = p.M;
    int rc;
    if (!y_ready) CK(e, run_norm(e, r.norm1, b.ln1w, b.ln1b, M, r.norm1_ld, b.oc_idx[0], r.noc, s));
    const uint16_t* qkv_w = weight_copy(r.qkv_wc, b.qkv_w, b.qkv_wp, b.qkv_wx);
    if (r.qkv == Gemm::FOLD) {
        CK(e, launch_gemm_et_fold(prec, e->Y, b.qkv_wf, e->QKV, b.qkv_bf, b.qkv_c, e->ROWSTAT, M, 3 * D, D, false, s));
    } else if (r.qkv == Gemm::MX) {
        CK(e, launch_gemm_et_mx(prec, e->Y, qkv_w, e->QKV, b.qkv_b, M, 3 * D, D, D, e->Y4[1], e->Y4[0], e->SY4[1], e->SY4[0],
                                b.qkv_w4[0], b.qkv_w4[1], b.qkv_s4[0], b.qkv_s4[1], false, false, r.v_from, s,
                                false, nullptr, nullptr, nullptr, nullptr, r.qkv_ld, r.noc != 0));
    } else if (r.qkv == Gemm::SPLIT3 && r.qkv_one) {
        CK(e, launch_gemm_et_split3(prec, e->Y, e->Ylo, b.qkv_w, b.qkv_w_lo, e->QKV, b.qkv_b, M, 3 * D, D, false, false, s, r.v_from));
    } else if (r.qkv == Gemm::SPLIT3) {
        if (!e->F32T) CK(e, dalloc(e, &e->F32T, (size_t)c.max_images * e->tokens * 4 * D));
        CK(e, gemm_hilo(prec, false, MainPass::LAST, e->Y, e->Ylo, b.qkv_w, b.qkv_w_lo, e->F32T, b.qkv_b, nullptr, 0, M, 3 * D, D, false, s));
        CK(e, launch_convert(prec, e->F32T, e->QKV, (long)M * 3 * D, s));
    } else {
        CK(e, launch_gemm_et(prec, e->Y, qkv_w, e->QKV, b.qkv_b, nullptr, 0, M, 3 * D, r.qkv_K, false, false, false, s, GemmOpts{r.qkv_ld, 1}));
    }
    if (!b.global)
        CK(e, launch_window_attention(prec, e->QKV, b.qkv_b, b.rel_h, b.rel_w, e->AO, n, g, c.window_size, c.num_heads, e->hd, s,
                                      r.ao_lo ? e->AOlo : nullptr, r.mx_ao ? e->AO4[0] : nullptr, r.mx_ao ? e->AO4[1] : nullptr,
                                      r.mx_ao ? e->SAO4[0] : nullptr, r.mx_ao ? e->SAO4[1] : nullptr, r.lo_heads));
    else
        CK(e, launch_global_attention(prec, e->QKV, b.rel_h, b.rel_w, e->AO, n, g, c.num_heads, e->hd, e->VTG, s,
                                      r.ao_lo ? e->AOlo : nullptr, r.mx_ao ? e->AO4[0] : nullptr, r.mx_ao ? e->AO4[1] : nullptr,
                                      r.mx_ao ? e->SAO4[0] : nullptr, r.mx_ao ? e->SAO4[1] : nullptr));
    // norm1 output (the live columns only: pad columns may hold an earlier pass's values), q | k | v, attention output
    if ((rc = range_scan(e, e->Y, (size_t)M * r.y1_live, s, r.y1_live, r.y1_ld))) return rc;
    if ((rc = range_scan(e, e->QKV, (size_t)M * 3 * D, s))) return rc;
    if ((rc = range_scan(e, e->AO, (size_t)M * D, s))) return rc;
    if ((rc = audit_site(e, AUDIT_PER_BLOCK * i + AUDIT_QKV_IN, e->Y, M, D, r.y1_ld, s))) return rc;
    for (int t = 0; t < 3; ++t)
        if ((rc = audit_site(e, AUDIT_PER_BLOCK * i + AUDIT_Q + t, e->QKV + (size_t)t * D, M, D, 3 * D, s))) return rc;
    if ((rc = audit_site(e, AUDIT_PER_BLOCK * i + AUDIT_PROJ_IN, e->AO, M, D, D, s))) return rc;

    if (r.proj == Gemm::FOLD) {
        CK(e, launch_gemm_et_stats(prec, e->AO, b.proj_w, e->X, b.proj_b, e->Y, e->STATS, M, D, D, s));
        CK(e, launch_ln_rowstat(e->STATS, e->ROWSTAT, M, 1e-6f, s));
    } else if (r.proj == Gemm::MX) {
        CK(e, launch_gemm_et_mx(prec, e->AO, b.proj_w, e->X, b.proj_b, M, D, D, e->mx_kp_proj, e->AO4[1], e->AO4[0], e->SAO4[1],
                                e->SAO4[0], b.proj_w4[0], b.proj_w4[1], b.proj_s4[0], b.proj_s4[1], true, true, 0, s));
    } else if (r.proj == Gemm::SPLIT3) {
        CK(e, gemm_hilo(prec, r.proj_one, MainPass::LAST, e->AO, e->AOlo, b.proj_w, b.proj_w_lo, e->X, b.proj_b, nullptr, 0, M, D, D, true, s));
    } else if (r.proj == Gemm::LNTAIL) {
        CK(e, launch_gemm_et_lntail(prec, e->AO, b.proj_w, e->X, b.proj_b, M, D, D, b.ln2w, b.ln2b, 1e-6f, e->Y, e->ln_counters, s));
    } else if (r.proj == Gemm::EXT) {
        CK(e, launch_outlier_gather(e->AO, e->AOlo, D, b.oc_idx[3], r.nop, e->OCX, M, s));
        CK(e, resid_gemm_ext(e, prec, e->AO, b.proj_w, e->OCX, b.oc_bx[3], b.proj_b, M, D, D, s));
    } else {
        CK(e, launch_gemm_et(prec, e->AO, b.proj_w, e->X, b.proj_b, nullptr, 0, M, D, D, true, false, true, s));
    }
    CK(e, run_norm(e, r.norm2, b.ln2w, b.ln2b, M, r.norm2_ld, b.oc_idx[1], r.nol, s));
    return SAMRS_OK;
}

// Second half of block i: lin1 (+ GELU) -> the scans of its operands -> lin2.
// *y_ready: set when norm1 of the next block came out of this block's lin2 launch (the next run_block_attn skips its LayerNorm)
static int run_block_mlp(samrs_engine_t* e, const PassRoute& p, const BlockRoute& r, const EncBlock& b, int i, bool* y_ready, hipStream_t s) {
    const int D = e->D, prec = e->prec, M = p.M;
    int rc;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (e->timing) {
        auto get = [&](hipEvent_t* ev) -> hipError_t {
            if (!e->tpool.empty()) { *ev = e->tpool.back(); e->tpool.pop_back(); return hipSuccess; }
            return hipEventCreate(ev);
        };
        CK(e, get(&t0)); CK(e, get(&t1));
        CK(e, hipEventRecord(t0, s));
    }
    if (r.lin1 == Gemm::FOLD) {
        CK(e, launch_gemm_et_fold(prec, e->Y, b.lin1_wf, e->H, b.lin1_bf, b.lin1_c, e->ROWSTAT, M, 4 * D, D, true, s));
    } else if (r.lin1 == Gemm::MX) {
        CK(e, launch_gemm_et_mx(prec, e->Y, b.lin1_w, e->H, b.lin1_b, M, 4 * D, D, D, e->Y4[1], e->Y4[0], e->SY4[1], e->SY4[0], b.lin1_w4[0],
                                b.lin1_w4[1], b.lin1_s4[0], b.lin1_s4[1], false, false, r.lin1_mx_from, s, true, e->H4[0], e->H4[1], e->SH4[0], e->SH4[1]));
    } else if (r.lin1 == Gemm::SPLIT3) {
        CK(e, gemm_hilo(prec, r.lin1_one, MainPass::LAST, e->Y, e->Ylo, b.lin1_w, b.lin1_w_lo, e->F32T, b.lin1_b, nullptr, 0, M, 4 * D, D, false, s));
        CK(e, launch_gelu_split(prec, e->F32T, e->H, e->Hlo, (long)M * 4 * D, s));
    } else {
        CK(e, launch_gemm_et(prec, e->Y, weight_copy(r.lin1_wc, b.lin1_w, b.lin1_wp, b.lin1_wx), e->H, b.lin1_b, nullptr, 0, M, 4 * D, r.lin1_K,
                             false, true, false, s, GemmOpts{r.lin1_ld, p.fast_gelu ? 2 : 1}));
    }
    if (e->timing) {
        CK(e, hipEventRecord(t1, s));
        e->tev.emplace_back(t0, t1);
    }
    // norm2 output (still in Y: lin1 has read it, nothing has overwritten it) and GELU(lin1)
    if ((rc = range_scan(e, e->Y, (size_t)M * r.y2_live, s, r.y2_live, r.y2_ld))) return rc;
    if ((rc = range_scan(e, e->H, (size_t)M * 4 * D, s))) return rc;
    if ((rc = audit_site(e, AUDIT_PER_BLOCK * i + AUDIT_LIN1_IN, e->Y, M, D, r.y2_ld, s))) return rc;
    if ((rc = audit_site(e, AUDIT_PER_BLOCK * i + AUDIT_LIN2_IN, e->H, M, 4 * D, 4 * D, s))) return rc;

    *y_ready = false;
    if (r.lin2 == Gemm::FOLD) {
        CK(e, launch_gemm_et_stats(prec, e->H, b.lin2_w, e->X, b.lin2_b, e->Y, e->STATS, M, D, 4 * D, s));
        if (r.next_rowstat) CK(e, launch_ln_rowstat(e->STATS, e->ROWSTAT, M, 1e-6f, s));
    } else if (r.lin2 == Gemm::MX) {
        CK(e, launch_gemm_et_mx(prec, e->H, b.lin2_w, e->X, b.lin2_b, M, D, 4 * D, e->mx_kp_lin2, e->H4[1], e->H4[0], e->SH4[1], e->SH4[0],
                                b.lin2_w4[0], b.lin2_w4[1], b.lin2_s4[0], b.lin2_s4[1], true, true, 0, s));
    } else if (r.lin2 == Gemm::SPLIT3) {
        CK(e, gemm_hilo(prec, r.lin2_one, MainPass::LAST, e->H, e->Hlo, b.lin2_w, b.lin2_w_lo, e->X, b.lin2_b, nullptr, 0, M, D, 4 * D, true, s));
    } else if (r.lin2 == Gemm::LNTAIL) {
        const EncBlock& nb = e->blocks[i + 1];
        CK(e, launch_gemm_et_lntail(prec, e->H, b.lin2_w, e->X, b.lin2_b, M, D, 4 * D, nb.ln1w, nb.ln1b, 1e-6f, e->Y, e->ln_counters, s));
        *y_ready = true;
    } else if (r.lin2 == Gemm::EXT) {
        CK(e, launch_outlier_side_gemm(prec, e->Y, r.side_ld, b.lin2_ws, b.lin2_sb, M, r.lin1_K, e->OCX, s));
        CK(e, resid_gemm_ext(e, prec, e->H, b.lin2_w, e->OCX, b.oc_bx[2], b.lin2_b, M, D, 4 * D, s));
    } else {
        CK(e, launch_gemm_et(prec, e->H, b.lin2_w, e->X, b.lin2_b, nullptr, 0, M, D, 4 * D, true, false, true, s));
    }
    return SAMRS_OK;
}

// layer-0 image side of slots [slot0, slot0 + n): see the K0F / K0E / KVQ0 members
static int prepare_slot_keys(samrs_engine_t* e, int slot0, int n, hipStream_t s) {
    const int C = e->C, Ci = C / 2, tokens = e->tokens, prec = e->prec;
    const DecLayer& L = e->layers[0];
    for (int i = 0; i < n; ++i) {
        const size_t o = (size_t)(slot0 + i) * tokens * C;
        CK(e, launch_make_keys(prec, e->EMB + o, nullptr, e->dec.no_mask_embed, e->K0F + o, e->K0E + o, 1, tokens, C, s));
    }
    CK(e, launch_gemm_et(prec, e->K0E + (size_t)slot0 * tokens * C, L.kvq_w, e->KVQ0 + (size_t)slot0 * tokens * 3 * Ci, L.kvq_b, L.kvq_pe,
                         tokens, n * tokens, 3 * Ci, C, false, false, false, s));
    return SAMRS_OK;
}

// neck: 1x1 conv -> LN2d -> 3x3 conv -> LN2d   (all channels-last), then the slots' layer-0 decoder keys.  Folded path: Y already is ET(X).
// SPLIT_NECK scratch: QKV (free after the last block) holds the lo halves.
static int run_neck(samrs_engine_t* e, const PassRoute& p, int n, int slot0, hipStream_t s) {
    const samrs_config& c = e->cfg;
    const int D = e->D, C = e->C, g = e->grid, tokens = e->tokens, prec = e->prec, M = p.M;
    const int audit_tail = AUDIT_PER_BLOCK * c.depth;
    int rc;
    uint16_t* lo_buf = e->QKV;
    if (p.sp_neck) CK(e, launch_convert(prec, e->X, e->Y, (long)M * D, s, lo_buf));
    else if (!(p.fold && c.depth > 0 && p.n_blocks >= c.depth)) CK(e, launch_convert(prec, e->X, e->Y, (long)M * D, s));
    // the RAW residual stream rounded to the operand type: the one operand without a LayerNorm in front
    if ((rc = range_scan(e, e->Y, (size_t)M * D, s))) return rc;
    if ((rc = audit_site(e, audit_tail + AUDIT_NECK1_IN, e->Y, M, D, D, s))) return rc;
    if (p.sp_neck)
        CK(e, gemm_hilo(prec, p.one3 && gemm_split3_ok(M, C, D, true), MainPass::FIRST, e->Y, lo_buf, e->neck0_w, e->neck0_w_lo, e->N1,
                        nullptr, nullptr, 0, M, C, D, false, s));
    else
        CK(e, launch_gemm_et(prec, e->Y, e->neck0_w, e->N1, nullptr, nullptr, 0, M, C, D, true, false, false, s));
    CK(e, launch_layernorm(prec, e->N1, W(e, "image_encoder.neck.1.weight"), W(e, "image_encoder.neck.1.bias"), 1e-6f,
                           e->N1e, nullptr, M, C, 0, g, 0, s, p.sp_neck ? lo_buf : nullptr));
    if ((rc = range_scan(e, e->N1e, (size_t)M * C, s))) return rc;
    if ((rc = audit_site(e, audit_tail + AUDIT_NECK2_IN, e->N1e, M, C, C, s))) return rc;
    CK(e, launch_neck_im2col(e->N1e, e->H, n, g, C, s));
    uint16_t* H2lo = e->H + (size_t)M * 9 * C;
    if (p.sp_neck) {
        CK(e, launch_neck_im2col(lo_buf, H2lo, n, g, C, s));
        CK(e, gemm_hilo(prec, p.one3 && gemm_split3_ok(M, C, 9 * C, true), MainPass::FIRST, e->H, H2lo, e->neck2_w, e->neck2_w_lo, e->N1,
                        nullptr, nullptr, 0, M, C, 9 * C, false, s));
    } else
        CK(e, launch_gemm_et(prec, e->H, e->neck2_w, e->N1, nullptr, nullptr, 0, M, C, 9 * C, true, false, false, s));
    CK(e, launch_layernorm(prec, e->N1, W(e, "image_encoder.neck.3.weight"), W(e, "image_encoder.neck.3.bias"), 1e-6f,
                           nullptr, e->EMB + (size_t)slot0 * tokens * C, M, C, 0, g, 0, s));
    return prepare_slot_keys(e, slot0, n, s);
}

// End of a full pass: the scans of the decoder's layer-0 keys, the range-check verdict, the audit countdown, the slot flags.
static int finish_pass(samrs_engine_t* e, const PassRoute& p, int n, int slot0, hipStream_t s) {
    const int C = e->C, tokens = e->tokens;
    int rc;
    if ((rc = range_scan(e, e->K0E + (size_t)slot0 * tokens * C, (size_t)n * tokens * C, s))) return rc;
    if (e->range_check == 2) {
        // fail loudly: this pass (and every earlier one since the last reset) must not have saturated an operand.  Costs a
        // stream synchronisation per encoder pass -- a validation mode for new checkpoints, not the production setting.
        unsigned long long now = 0;
        CK(e, hipStreamSynchronize(s));
        CK(e, hipMemcpy(&now, e->range_counter, sizeof(now), hipMemcpyDeviceToHost));
        const unsigned long long before = e->range_seen;
        e->range_seen = now;
        if (now > before)
            return fail(e, SAMRS_ERR_RANGE, "%llu operand values of this encoder pass saturated the %s range (|x| >= %s): the masks of these "
                        "images are not the reference's.  Use precision bf16 (fp32 exponent range, 8 mantissa bits) for this "
                        "checkpoint, or option \"range_check\" = 1 to count without failing", now - before,
                        e->prec == PREC_F16 ? "f16" : "bf16", e->prec == PREC_F16 ? "65504" : "inf");
    }
    if ((rc = audit_site(e, AUDIT_PER_BLOCK * e->cfg.depth + AUDIT_KEYS0, e->K0E + (size_t)slot0 * tokens * C, p.M, C, C, s))) return rc;
    // "audit_passes": a full pass has been profiled; after the last one the profile switches itself off
    if (e->audit_passes > 0 && --e->audit_passes == 0) e->range_profile = 0;
    for (int i = 0; i < n; ++i) {
        e->slot_set[slot0 + i] = 1;
        e->slot_split[slot0 + i] = e->split;
        e->slot_depth[slot0 + i] = (e->split & (SPLIT_ATTN | SPLIT_MLP | SPLIT_LIN2)) ? p.depth_full : (e->split & SPLIT_ATTN_V) ? p.depth_v : 0;
    }
    return SAMRS_OK;
}

// -------------------------------------------------------------------------------------------------
// images[i]: device pointer of tile i (uint8 HWC, in_h[i] x in_w[i], long side == img_size).  Tiles of one call may
// differ in size (HRSC / DIOR images after ResizeLongestSide): only the im2col reads pixels, everything downstream
// works on the zero-padded 64 x 64 token grid (sam.py:170-173).
static int encode(samrs_engine_t* e, const uint8_t* const* images, const int* in_h, const int* in_w, int n, int slot0,
                  void* stream, int n_blocks, bool do_neck) {
    if (!e || !images || !in_h || !in_w) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_set_images: null argument");
    if (!e->finalized) return fail(e, SAMRS_ERR_BAD_WEIGHTS, "weights not finalized");
    const samrs_config& c = e->cfg;
    if (n < 1 || slot0 < 0 || slot0 + n > c.max_images) return fail(e, SAMRS_ERR_CAPACITY, "n_images/slot out of range (max_images=%d)", c.max_images);
    for (int i = 0; i < n; ++i) {
        if (!images[i]) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_set_images: null image pointer (tile %d)", i);
        if (in_h[i] < 1 || in_w[i] < 1 || in_h[i] > c.img_size || in_w[i] > c.img_size || (in_h[i] != c.img_size && in_w[i] != c.img_size))
            return fail(e, SAMRS_ERR_BAD_SHAPE, "set_torch_image input must be BCHW with long side %d.", c.img_size);
    }
    hipStream_t s = (hipStream_t)stream;
    ON_DEVICE(e);
    int rc;
    for (int i = 0; i < n; ++i) e->slot_set[slot0 + i] = 0;
    if (e->range_profile && (rc = audit_prepare(e, e->range_profile == 2))) return rc;
    const PassRoute p = pass_route(e, n * e->tokens, n_blocks);
    if ((rc = run_patch_embed(e, p, images, in_h, in_w, n, s))) return rc;
    bool y_ready = false;          // Y already holds norm1 of the block about to start (written by the previous block's lin2 launch)
    for (int i = 0; i < c.depth && i < n_blocks; ++i) {
        const EncBlock& b = e->blocks[i];
        const BlockRoute r = block_route(e, p, b, i);
        if ((rc = run_block_attn(e, p, r, b, i, n, y_ready, s))) return rc;
        if ((rc = run_block_mlp(e, p, r, b, i, &y_ready, s))) return rc;
    }
    if (!do_neck) return SAMRS_OK;         // samrs_debug_encoder_prefix: no slot is set and the pass does not count as profiled
    if ((rc = run_neck(e, p, n, slot0, s))) return rc;
    return finish_pass(e, p, n, slot0, s);
}

// a contiguous stack of same-size tiles as encode()'s pointer table.  The two checks here are what building the table needs (a bounded n,
// which takes the engine; a base pointer to offset); encode() validates everything else, the sizes included
static int encode_stack(samrs_engine_t* e, const uint8_t* images, int n, int in_h, int in_w, int slot0, void* stream,
                        int n_blocks, bool do_neck) {
    if (!e || !images) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_set_images: null argument");
    if (n < 1 || n > e->cfg.max_images) return fail(e, SAMRS_ERR_CAPACITY, "n_images/slot out of range (max_images=%d)", e->cfg.max_images);
    std::vector<const uint8_t*> ptr(n);
    std::vector<int> hs(n, in_h), ws(n, in_w);
    for (int i = 0; i < n; ++i) ptr[i] = images + (size_t)i * (in_h > 0 ? in_h : 0) * (in_w > 0 ? in_w : 0) * 3;
    return encode(e, ptr.data(), hs.data(), ws.data(), n, slot0, stream, n_blocks, do_neck);
}

extern "C" {
int samrs_set_images(samrs_engine_t* e, const uint8_t* images, int n, int in_h, int in_w, int slot0, void* stream) {
    return encode_stack(e, images, n, in_h, in_w, slot0, stream, 1 << 30, true);
}

int samrs_set_images_ragged(samrs_engine_t* e, const uint8_t* const* images, const int* in_h, const int* in_w, int n,
                            int slot0, void* stream) {
    return encode(e, images, in_h, in_w, n, slot0, stream, 1 << 30, true);
}

int samrs_debug_encoder_prefix(samrs_engine_t* e, const uint8_t* images, int n, int in_h, int in_w, int n_blocks,
                               float* x_out, void* stream) {
    if (!x_out) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_debug_encoder_prefix: null output");
    const int rc = encode_stack(e, images, n, in_h, in_w, 0, stream, n_blocks, false);
    if (rc) return rc;
    CK(e, hipMemcpyAsync(x_out, e->X, sizeof(float) * (size_t)n * e->tokens * e->D, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SAMRS_OK;
}

int samrs_get_embedding(samrs_engine_t* e, int slot, float* out_chw, void* stream) {
    if (!e || !out_chw) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_get_embedding: null argument");
    if (slot < 0 || slot >= e->cfg.max_images) return fail(e, SAMRS_ERR_CAPACITY, "slot out of range");
    if (!e->slot_set[slot]) return fail(e, SAMRS_ERR_NOT_SET, "An image must be set with .set_image(...) to generate an embedding.");
    ON_DEVICE(e);
    CK(e, launch_transpose_f32(e->EMB + (size_t)slot * e->tokens * e->C, out_chw, e->tokens, e->C, (hipStream_t)stream));
    return SAMRS_OK;
}

int samrs_set_embedding(samrs_engine_t* e, int slot, const float* emb_chw, void* stream) {
    if (!e || !emb_chw) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_set_embedding: null argument");
    if (!e->finalized) return fail(e, SAMRS_ERR_BAD_WEIGHTS, "weights not finalized");
    if (slot < 0 || slot >= e->cfg.max_images) return fail(e, SAMRS_ERR_CAPACITY, "slot out of range");
    ON_DEVICE(e);
    CK(e, launch_transpose_f32(emb_chw, e->EMB + (size_t)slot * e->tokens * e->C, e->C, e->tokens, (hipStream_t)stream));
    { const int rc = prepare_slot_keys(e, slot, 1, (hipStream_t)stream); if (rc != SAMRS_OK) return rc; }
    e->slot_set[slot] = 1;
    e->slot_split[slot] = -1;
    e->slot_depth[slot] = 0;
    return SAMRS_OK;
}

// ---- checkpoint audit: the public reads (samrs_hip.h)
int samrs_audit_site_count(const samrs_engine_t* e, int* n_sites) {
    if (!e || !n_sites) return SAMRS_ERR_BAD_ARG;
    *n_sites = (int)e->audit_sites.size();
    return SAMRS_OK;
}
int samrs_audit_site_name(const samrs_engine_t* e, int site, char* name, int name_len, int* columns) {
    if (!e || !name || name_len < 1 || site < 0 || site >= (int)e->audit_sites.size()) return SAMRS_ERR_BAD_ARG;
    snprintf(name, (size_t)name_len, "%s", e->audit_sites[site].name.c_str());
    if (columns) *columns = e->audit_sites[site].columns;
    return SAMRS_OK;
}
int samrs_audit_read_profile(samrs_engine_t* e, int64_t* rows, int reset) {
    if (!e || !rows) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_audit_read_profile: null argument");
    const size_t n = e->audit_sites.size() * AUDIT_PROFILE_WORDS;
    if (!e->audit_rows) {                  // nothing profiled yet
        for (size_t i = 0; i < n; ++i) rows[i] = 0;
        return SAMRS_OK;
    }
    ON_DEVICE(e);
    CK(e, hipDeviceSynchronize());
    CK(e, hipMemcpy(rows, e->audit_rows, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return reset ? audit_reset(e) : SAMRS_OK;
}
int samrs_audit_read_columns(samrs_engine_t* e, int site, double* sumsq, float* max_abs, int64_t* n_rows) {
    if (!e || !sumsq || !max_abs || !n_rows) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_audit_read_columns: null argument");
    if (site < 0 || site >= (int)e->audit_sites.size()) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_audit_read_columns: site %d of %d", site, (int)e->audit_sites.size());
    const samrs_engine::AuditSite& a = e->audit_sites[site];
    if (a.columns == 0)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_audit_read_columns: site %s has no column statistics (the block GEMMs' A operands have: qkv_in, proj_in, lin1_in, lin2_in)", a.name.c_str());
    if (!e->audit_sumsq || e->audit_col_rows[site] == 0)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_audit_read_columns: no encoder pass has been profiled with option \"range_profile\" = 2 (or \"audit_passes\") since the last reset");
    ON_DEVICE(e);
    CK(e, hipDeviceSynchronize());
    std::vector<uint32_t> bits((size_t)a.columns);
    CK(e, hipMemcpy(sumsq, e->audit_sumsq + a.col_off, sizeof(double) * a.columns, hipMemcpyDeviceToHost));
    CK(e, hipMemcpy(bits.data(), e->audit_maxbits + a.col_off, sizeof(uint32_t) * a.columns, hipMemcpyDeviceToHost));
    for (int c = 0; c < a.columns; ++c) {
        uint32_t u;                        // the operand type's magnitude pattern as fp32 bits
        if (e->prec == PREC_BF16) u = bits[c] << 16;
        else {
            const uint32_t ex = bits[c] >> 10, m = bits[c] & 0x3ffu;
            if (ex == 31) u = 0x7f800000u | (m << 13);
            else if (ex) u = ((ex + 112) << 23) | (m << 13);
            else { const float f = (float)m * 5.9604644775390625e-8f /* 2^-24 */; memcpy(&u, &f, 4); }
        }
        memcpy(&max_abs[c], &u, 4);
    }
    *n_rows = (int64_t)e->audit_col_rows[site];
    return SAMRS_OK;
}
}  // extern "C"
