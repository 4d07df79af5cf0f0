// gemm_select.h -- which kernel runs a 16-bit GEMM launch (launch_gemm_et): the one statement of the rule.
// Plain C++17: no HIP, no environment, no globals.  gemm.hip builds a GemmCall / GemmEnv per launch and switches on the answer;
// the planning predicates the engine asks (gemm_ld_ok, gemm_ext_ok, gemm_lntail_ok) are statements about the same answer.
#pragma once

namespace gemm_sel {

// tile shapes of the kernels the rule chooses between (the kernels themselves: gemm.hip)
constexpr int BM = 128, BN = 128, BK = 64;                  // base 128 x 128 tile; every launch is whole tiles of it
constexpr int PBM = 256;                                    // staggered kernel: 256 x 128
constexpr int DBM = 256, DBN = 128, DBK = 32;               // dual (2 blocks / CU) kernel
constexpr int QBM = 256, QBN = 256, QBK = 32;               // 256 x 256 staggered kernel, 32-deep ring
constexpr int WBN = 320;                                    // its NI = 5 flavour and the pair-stage kernels: 256 x 320
constexpr int XBK = 64;                                     // pair-stage kernels: 64-k stages
constexpr int W4X_BN = 256;                                 // four-wave kernel: 256 x 256
constexpr int K2_ROWS = 128, K2_K = 256;                    // K = 256 streaming kernel: 128-row tiles

// one enumerator per launcher (launch_gemm_* in gemm.hip)
enum class GemmKernel {
    BASE,            // launch_gemm_prec<glds, group_m>: 128 x 128, any valid shape
    STAG,            // launch_gemm_stag: 256 x 128, staggered wave groups
    DUAL,            // launch_gemm_dual: 2 blocks / CU
    DUAL_LOCKSTEP,   // launch_gemm_dual<STAG = false>: one barrier per K step
    STAG_256x256,    // launch_gemm_big<4>
    STAG_256x320,    // launch_gemm_big<5>
    X64,             // launch_gemm_x64<ni, mode>: pair-stage, one tile per block
    X64P,            // launch_gemm_x64p: pair-stage, persistent
    W4X,             // launch_gemm_w4x: four waves, 256 x 256, persistent
    K256,            // launch_gemm_k256: K = 256 streaming
    // make EXPERIMENTS=1 only: measured and not adopted
    M32,             // launch_gemm_m32<mode = spread>: 32x32x16 symmetric schedule
    W4,              // launch_gemm_w4: its four-wave flavour
    ABL_BIG,         // gemm_et_big_kernel<abl>: timing ablations 60 + abl
    ABL_X64,         // gemm_et_x64_kernel<5, 3, abl>: timing ablations 100 + abl
};

struct GemmCall {            // what the caller asks for
    int M, N, K;
    bool out_f32, gelu, accumulate, has_add2d;
    int ld;                  // operand row stride in elements, 0 = K
    bool f16;                // the rule looks at the precision only here: the ablation families exist in f16 alone
};
struct GemmEnv {             // read once from the process
    int variant;             // the engine's thread-local override if set, else the process-wide one (SAMRS_GEMM_VARIANT, 8 = automatic)
    bool w4x_auto;           // SAMRS_GEMM_W4X != 0 (default on): the automatic rule may pick the four-wave kernel
    int m32_mask;            // SAMRS_GEMM_M32 (experiments builds): see below
    bool experiments;        // the build has the experiment kernels
};
struct GemmChoice {
    GemmKernel kernel = GemmKernel::BASE;
    int ni = 0, mode = 0;    // X64: N tile = 64 ni, schedule mode; M32: mode = spread pieces
    bool glds = true;        // BASE: LDS-DMA staging
    int group_m = 8;         // BASE: grouped tile order
    bool persistent = false; // M32 / W4: one block per CU walks the tiles
    int abl = 0;             // ABL_*: which ablation
    bool reject = false;     // hipErrorInvalidValue, nothing launched
};

// the shapes each kernel with a narrower domain takes
inline bool w4x_ok(int M, int N, int K, bool has_add2d, bool out_f32) {
    return M % QBM == 0 && N % W4X_BN == 0 && K % XBK == 0 && K >= 4 * XBK && !has_add2d && !out_f32;
}
inline bool m32_ok(int M, int N, int K, bool has_add2d) {
    return M % QBM == 0 && N % WBN == 0 && K % (2 * XBK) == 0 && K >= 2 * XBK && !has_add2d;
}
// the streaming kernel: ET output without GELU / accumulate, K = 256, N = 256 or 384, whole 128-row tiles
inline bool k256_ok(int M, int N, int K, bool out_f32, bool gelu, bool accumulate) {
    return !out_f32 && !gelu && !accumulate && K == K2_K && (N == 256 || N == 384) && M % K2_ROWS == 0;
}
inline bool x64_ok(int M, int N, int K, int ni) { return M % QBM == 0 && N % (64 * ni) == 0 && K % XBK == 0; }

// Variant 8 ("auto", default): per-shape pick measured on MI355X (tools/gemm_bench.py) -- the 2-blocks-per-CU kernel wins where the
// epilogue dominates (GELU output, or short K with a narrow N), the 64-wide-K single-block kernel wins on long K / wide N.
// Returns the numbered variant to go on with: 5, 6, 7, 10, 27 or 28.
inline int gemm_auto_variant(const GemmCall& c) {
    const bool big_ok = c.M % QBM == 0 && c.K % QBK == 0;
    const long t256 = big_ok && c.N % QBN == 0 ? (long)(c.M / QBM) * (c.N / QBN) : 0;
    const long t320 = big_ok && c.N % WBN == 0 ? (long)(c.M / QBM) * (c.N / WBN) : 0;
    // the 256x320 tile: pair-stage kernel (whole-line DMA, one barrier per 64 k, DMA pieces spread between the MFMAs;
    // measured +1.5 ... +4 % over the 32-deep ring on all four encoder shapes, bit-identical) when K allows, else
    // the 32-deep staggered kernel
    const int wide = (c.K % XBK == 0) ? 27 : 10;
    // fp32 residual outputs (proj, lin2: N = 1280): 256x320 tiles -> an exact number of rounds over the 256 CUs
    if (c.out_f32 && t320 >= 256) return wide;
    // f16 outputs (qkv N = 3840, lin1+GELU N = 5120): the wide tile whenever it fills whole rounds (6 / 8 rounds at
    // batch 8, exactly one round for lin1 of a single image), else 256x256 as long as there are >= 4 rounds of tiles
    // (ET outputs without a 2-D addend: the persistent flavour, +3 % on qkv / lin1; its one-m-tile fp32 epilogue loses on proj)
    if (!c.out_f32 && t320 >= 256 && t320 % 256 == 0) return (wide == 27 && !c.has_add2d) ? 28 : wide;
    if (!c.out_f32 && c.N >= 2048 && t256 >= 1024) return 6;
    return (c.gelu || (c.K <= 1536 && c.N <= 1536)) ? 7 : 5;
}

// the rule proper, for a call that passed gemm_select's shape checks
inline GemmChoice gemm_rule(const GemmCall& c, const GemmEnv& e) {
    using GK = GemmKernel;
    const int M = c.M, N = c.N, K = c.K, gv = e.variant;
    auto pick = [](GK k) { GemmChoice ch; ch.kernel = k; return ch; };
    auto rejected = [] { GemmChoice ch; ch.reject = true; return ch; };
    const bool x64p_fits = x64_ok(M, N, K, 5) && !c.has_add2d;

    // 60 + abl: ablations of the 256x256 staggered kernel (f16, ET output): timing experiments only
    if (e.experiments && gv >= 60 && gv < 92 && c.f16 && !c.out_f32 && M % QBM == 0 && N % QBN == 0) {
        GemmChoice ch = pick(GK::ABL_BIG);
        ch.abl = gv - 60;
        for (int a : {0, 1, 4, 6, 8, 7, 16, 22, 23, 24}) if (a == ch.abl) return ch;
        return rejected();
    }
    // 40: K = 256 streaming kernel (decoder image side); automatic for its shapes once there are >= 2 tiles per CU
    if ((gv == 40 || (gv == 8 && M / K2_ROWS >= 512)) && k256_ok(M, N, K, c.out_f32, c.gelu, c.accumulate)) return pick(GK::K256);

    int v = gv;
    // 28 (persistent pair-stage) on a shape it does not cover: the automatic choice
    if (v == 28 && !x64p_fits) v = 8;
    // 20 ... 27, 35: pair-stage (64-deep, whole-cache-line DMA) kernel, one tile per block: 20 + 2 mode + (NI == 5), mode bit 0 = spread
    // DMA, bit 1 = one barrier per stage; 35 = mode 7 at NI = 5.  Shapes they do not cover: the automatic choice
    if ((v >= 20 && v <= 27) || v == 35) {
        GemmChoice ch = pick(GK::X64);
        ch.ni = (v & 1) ? 5 : 4;
        ch.mode = v == 35 ? 7 : (v - 20) >> 1;
        if (x64_ok(M, N, K, ch.ni)) return ch;
        v = 8;
    }
    // 100 + abl: ablations of the barrier-light 256x320 kernel (f16, ET output, no GELU): timing experiments only
    if (e.experiments && v >= 100 && v < 196 && c.f16 && !c.out_f32 && x64_ok(M, N, K, 5)) {
        GemmChoice ch = pick(GK::ABL_X64);
        ch.abl = v - 100;
        for (int a : {0, 1, 2, 4, 16, 6, 7, 22, 23, 17, 32, 33, 64}) if (a == ch.abl) return ch;
        return rejected();
    }
    if (v == 8) v = gemm_auto_variant(c);

    // ET + GELU outputs whose 256 x 256 tiles fill whole rounds (lin1 of ViT-H: 2560 tiles = 10 rounds at batch 8; 5 at batch 4) go to
    // the four-wave 128 x 128-wave-tile kernel (variant 38; bit-identical with the kernel it replaces, so no mode's arithmetic moves).
    // Measured on MI355X: as a 2.5 s loop of its own 412 us against 429 and 1.03 against 1.08 pJ / FLOP (profiles/r05_gemm_energy.txt);
    // INSIDE the tile loop, beside the decoder's kernels, the launch itself is no faster (0.4342 against 0.4330 ms) and the step gains
    // 0.2 % (142.68 / 142.68 / 142.88 against 142.21 / 142.57 / 142.52 images/s, alternated on one box: profiles/r05_ab_loop.txt).
    // Plain ET outputs (qkv: 7.5 rounds) and the fp32 outputs (2.5 rounds) are slower on it in both settings and stay where they were.
    // SAMRS_GEMM_W4X=0 switches the rule off (A/B runs).
    if (v == 28 && e.w4x_auto && c.gelu && w4x_ok(M, N, K, c.has_add2d, c.out_f32)) {
        const long t256 = (long)(M / QBM) * (N / W4X_BN);
        if (t256 % 256 == 0 && t256 >= 1024) v = 38;
    }
    // SAMRS_GEMM_M32=<mask> lets the automatic rule pick the 32x32x16 kernels for A/B runs of the whole loop: bit 0 = ET outputs (qkv,
    // lin1), bit 1 = fp32 outputs (proj, lin2), bit 2 = one tile per block instead of persistent, bit 3 = spread pieces, bit 4 = the
    // four-wave flavour.  They take no operand stride.
    if (e.experiments && (v == 27 || v == 28) && c.ld == 0 && m32_ok(M, N, K, c.has_add2d) && (e.m32_mask & (c.out_f32 ? 2 : 1)))
        v = (e.m32_mask & 16) ? 34 : 30 + ((e.m32_mask & 4) ? 1 : 0) + ((e.m32_mask & 8) ? 2 : 0);

    const int pair = c.has_add2d ? 27 : 28;     // where 30 ... 38 fall back to
    // 30 ... 36 in a build without them, or on a shape they do not cover: the pair-stage kernel
    if (v >= 30 && v <= 36 && !(e.experiments && m32_ok(M, N, K, c.has_add2d))) v = pair;
    // 30 / 31: 32x32x16 symmetric-schedule kernel, persistent / one tile per block, all pieces in step 3; 32 / 33: pieces spread over two
    if (v >= 30 && v <= 33) {
        GemmChoice ch = pick(GK::M32);
        ch.mode = v >= 32;
        ch.persistent = !(v & 1);
        return ch;
    }
    // 34 / 36: the four-wave, 512-register flavour of the symmetric schedule (persistent / one tile per block)
    if (v == 34 || v == 36) {
        GemmChoice ch = pick(GK::W4);
        ch.persistent = v == 34;
        return ch;
    }
    // 38: the four-wave 256 x 256 kernel on 16x16x32 MFMAs with 128 x 128 wave tiles; shapes it does not cover: the pair-stage kernel
    if (v == 38 && !w4x_ok(M, N, K, c.has_add2d, c.out_f32)) v = pair;
    if (v == 38) return pick(GK::W4X);
    if (v == 28 && x64p_fits) return pick(GK::X64P);
    // 28 with a 2-D addend, 27 from the automatic rule: one tile per block, mode 3
    if ((v == 28 || v == 27) && x64_ok(M, N, K, 5)) {
        GemmChoice ch = pick(GK::X64);
        ch.ni = 5;
        ch.mode = 3;
        return ch;
    }
    const bool dual_fits = M % DBM == 0 && K % DBK == 0;
    if (v == 9 && dual_fits) return pick(GK::DUAL_LOCKSTEP);
    if (v == 7 && dual_fits) return pick(GK::DUAL);
    // 10 (11: the round-1 persistent 32-deep kernel was removed, 28 is its successor): 256x320 staggered kernel, else the 256x128 one
    if ((v == 10 || v == 11) && M % QBM == 0 && N % WBN == 0 && K % QBK == 0) return pick(GK::STAG_256x320);
    if (v == 10 || v == 11) v = 5;
    if (v == 6 && M % QBM == 0 && N % QBN == 0 && K % QBK == 0) return pick(GK::STAG_256x256);
    // 5, and 6 / 7 / 9 on shapes they do not cover
    if ((v == 5 || v == 6 || v == 7 || v == 9) && M % PBM == 0) return pick(GK::STAG);
    // everything else: the 128 x 128 kernel; 0 register-staged, 1 + LDS-DMA, 3 register-staged + grouped order, otherwise both
    GemmChoice ch = pick(GK::BASE);
    ch.glds = !(gv == 0 || gv == 3);
    ch.group_m = (gv == 0 || gv == 1) ? 1 : 8;
    return ch;
}

inline bool gemm_takes_ld(GemmKernel k) { return k == GemmKernel::X64P || k == GemmKernel::W4X; }

inline GemmChoice gemm_select(const GemmCall& c, const GemmEnv& e) {
    GemmChoice no;
    no.reject = true;
    if (c.M <= 0 || c.N <= 0 || c.K <= 0 || c.M % BM || c.N % BN || c.K % BK) return no;
    if (c.has_add2d && c.gelu) return no;   // not needed by the path; the coalesced epilogue orders them differently
    const GemmChoice ch = gemm_rule(c, e);
    // a padded operand stride is understood by the persistent ET kernels only, and planned for (gemm_ld_ok) under the automatic rule
    // only: refuse anything else instead of reading garbage.  Both kernels fetch a row's k-slice as 16-byte LDS-DMA pieces at byte offset
    // 2 (row ld + 8 chunk) from a 16-byte-aligned base (gemm.hip voff / voffq): a stride that is no multiple of 8 elements would put
    // every odd row's pieces off their 16-byte alignment, so it is refused too
    if (c.ld != 0 && (c.ld < c.K || c.ld % 8 || e.variant != 8 || c.out_f32 || c.has_add2d || !gemm_takes_ld(ch.kernel))) return no;
    return ch;
}

// ---- what the engine plans with: statements about the rule's answer.  Asked of the rule proper: the whole-tile checks of a plain launch
// stay the launch's (the EXT / LayerNorm-tail launches are whole 256 x 320 tiles, not 128 x 128 ones; the engine only has widths that are
// both: embed_dim % 128 == 0), and the A/B mask redirects launches, not plans.
inline bool gemm_is_x64_wide(const GemmChoice& ch) { return !ch.reject && ch.kernel == GemmKernel::X64 && ch.ni == 5 && ch.mode == 3; }
inline GemmChoice gemm_plan_choice(int M, int N, int K, bool out_f32, bool gelu, bool accumulate, GemmEnv e) {
    e.m32_mask = 0;
    return gemm_rule(GemmCall{M, N, K, out_f32, gelu, accumulate, false, 0, true}, e);
}
// a plain ET launch of this shape runs on one of the two kernels that take an operand row stride
inline bool gemm_plan_ld_ok(int M, int N, int K, bool gelu, const GemmEnv& e) {
    const GemmChoice ch = gemm_plan_choice(M, N, K, false, gelu, false, e);
    return e.variant == 8 && !ch.reject && gemm_takes_ld(ch.kernel);
}
// fp32 residual outputs with the outlier-column stage (one more 64-k stage: K >= 2 stages): the shapes the one-tile 256 x 320 pair-stage
// kernel takes by the automatic rule
inline bool gemm_plan_ext_ok(int M, int N, int K, const GemmEnv& e) {
    return e.variant == 8 && K >= 2 * XBK && gemm_is_x64_wide(gemm_plan_choice(M, N, K, true, false, true, e));
}
// ... and with the LayerNorm tail: the same shapes whatever variant is forced, N one LayerNorm row of at most 1280
inline bool gemm_plan_lntail_ok(int M, int N, int K, GemmEnv e) {
    e.variant = 8;
    return N <= 1280 && K >= 2 * XBK && gemm_is_x64_wide(gemm_plan_choice(M, N, K, true, false, true, e));
}

}  // namespace gemm_sel
