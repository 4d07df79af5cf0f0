// gemm_dual.hip -- gemm_et_dual_kernel: the gemm_et kernel of which two blocks fit a CU (what gemm_et computes: gemm.hip), and its
// GELU(LayerNorm2d) flavour behind launch_gemm_et_gln.
#include "gemm_device.h"
#include "gemm_families.h"

namespace {

// ---------------------------------------------------------------------------------------------
// gemm_et_dual_kernel: the staggered 256x128 kernel with a 32-wide K step: three 24 KiB ring stages
// = 72 KiB of LDS and <= 128 VGPRs, so TWO blocks (16 waves) are resident per CU and one block's
// epilogue (HBM-write bound: up to a third of the single-block kernel, ablation in DESIGN.md)
// overlaps the other block's main loop.  Per K step and wave: 3 DMA pieces, 8 ds_read_b128,
// 16 MFMAs, two raw barriers (L | C segments, wave groups staggered by one interval).
// ---------------------------------------------------------------------------------------------
constexpr int DSTAGES = 3, DTHREADS = 512;
constexpr int DSTAGE_ELEMS = (DBM + DBN) * DBK;               // 12288 ET = 24 KiB
constexpr int D_DMA_PER_TILE = (DBM + DBN) * DBK * 2 / (DTHREADS * 16);   // 3 per thread

// SPLIT: both operands come as hi + lo (two-term split, common.h) and the k loop runs three times over K:
// A_lo B_hi, A_hi B_lo, A_hi B_hi (small terms first), all into the same fp32 accumulators -- the product of the
// un-rounded operands to ~2^-22 at three times the MFMA work.  Used for the decoder's first transposed conv, whose
// operand rounding cost 376 of the 899 class-map pixels of the round-2 engine at ViT-H (oracle/error_budget.py).
template <int PREC, bool OUT_F32, bool GELU, bool STAG = true, bool GLN = false, bool SPLIT = false>
__global__ __launch_bounds__(DTHREADS, 4) void gemm_et_dual_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, void* __restrict__ Cv,
    const float* __restrict__ bias, const float* __restrict__ add2d, int add2d_period,
    int M, int N, int K, int accumulate, const uint16_t* __restrict__ A_lo = nullptr, const uint16_t* __restrict__ B_lo = nullptr) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[DSTAGES * DSTAGE_ELEMS];   // 72 KiB, ONE object

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;
    const int wm = wave >> 1, wn = wave & 1;

    constexpr int GROUP = 8;
    const int tiles_n = N / DBN, tiles_m = M / DBM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int per_group = GROUP * tiles_n;
    const int group = bid / per_group, first_m = group * GROUP;
    const int gsz = (tiles_m - first_m) < GROUP ? (tiles_m - first_m) : GROUP;
    const int in_g = bid - group * per_group;
    const int tile_m = first_m + in_g % gsz, tile_n = in_g / gsz;
    const int m0 = tile_m * DBM, n0 = tile_n * DBN;

    // DMA: piece = 16 rows x 64 B; lane l -> row l>>2, physical chunk l&3 (source chunk swizzled).
    // wave w: A rows 16w.. and 128+16w.., B rows 16w..
    const int g_row = 16 * wave + (lane >> 2);
    const int g_chunk = qswz(g_row, lane & 3);
    const uint16_t* gAg = A + (size_t)(m0 + g_row) * K + g_chunk * 8;
    const uint16_t* gBg = B + (size_t)(n0 + g_row) * K + g_chunk * 8;
    const uint16_t* gAl = SPLIT ? A_lo + (size_t)(m0 + g_row) * K + g_chunk * 8 : gAg;
    const uint16_t* gBl = SPLIT ? B_lo + (size_t)(n0 + g_row) * K + g_chunk * 8 : gBg;
    const uint32_t wave_lds_base = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds + (uint32_t)wave * (16 * DBK * 2));
    const size_t rs128 = (size_t)128 * K;
    const int nk1 = K / DBK;                   // k tiles of one pass over K
#define DUAL_ISSUE(kt_, stage_)                                                                 \
    do {                                                                                         \
        const int ph_ = SPLIT ? (kt_) / nk1 : 2;       /* 0: A_lo B_hi, 1: A_hi B_lo, 2: A_hi B_hi */ \
        const size_t koff_ = (size_t)((kt_) - (SPLIT ? ph_ * nk1 : 0)) * DBK;                    \
        const uint16_t* pa_ = ph_ == 0 ? gAl : gAg;                                              \
        const uint16_t* pb_ = ph_ == 1 ? gBl : gBg;                                              \
        constexpr int SB_ = (stage_) * DSTAGE_ELEMS * 2;                                         \
        glds16_asm<SB_ + 0>(pa_ + koff_, wave_lds_base);                                         \
        glds16_asm<SB_ + 128 * DBK * 2>(pa_ + rs128 + koff_, wave_lds_base);                     \
        glds16_asm<SB_ + DBM * DBK * 2>(pb_ + koff_, wave_lds_base);                             \
    } while (0)

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nk = nk1 * (SPLIT ? 3 : 1);
    DUAL_ISSUE(0, 0);
    if (nk > 1) {
        DUAL_ISSUE(1, 1);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D_DMA_PER_TILE) : "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    if (STAG && grp == 1) __builtin_amdgcn_s_barrier();          // stagger

    const int fr = lane & 15, fq = lane >> 4;
    int offA[4], offB[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int r = wm * 64 + j * 16 + fr; offA[j] = r * DBK + qswz(r, fq) * 8; }
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int r = wn * 64 + i * 16 + fr; offB[i] = DBM * DBK + r * DBK + qswz(r, fq) * 8; }

#define DUAL_WAIT(kt_)                                                                           \
    if ((kt_) + 2 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(D_DMA_PER_TILE) : "memory");     \
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#define DUAL_STEP(kt_, S_)                                                                       \
    if ((kt_) < nk) {                                                                            \
        uint4 fa[4], fb[4];                                                                      \
        if ((kt_) + 2 < nk) DUAL_ISSUE((kt_) + 2, ((S_) + 2) % DSTAGES);                         \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                            \
            fb[i] = *reinterpret_cast<const uint4*>(lds + (S_) * DSTAGE_ELEMS + offB[i]);        \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                            \
            fa[j] = *reinterpret_cast<const uint4*>(lds + (S_) * DSTAGE_ELEMS + offA[j]);        \
        if (STAG) {                                                                              \
        DUAL_WAIT(kt_)                                                                           \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                       \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        __builtin_amdgcn_s_barrier();                                                            \
        }                                                                                        \
        __builtin_amdgcn_s_setprio(1);                                                           \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                            \
            _Pragma("unroll") for (int j = 0; j < 4; ++j)                                        \
                acc[i][j] = ET<PREC>::mfma16(fb[i], fa[j], acc[i][j]);                           \
        __builtin_amdgcn_s_setprio(0);                                                           \
        DUAL_WAIT(kt_)                                                                           \
        if (!STAG) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                            \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        __builtin_amdgcn_s_barrier();                                                            \
    }
    for (int kt = 0; kt < nk; kt += DSTAGES) {
        DUAL_STEP(kt, 0)
        DUAL_STEP(kt + 1, 1)
        DUAL_STEP(kt + 2, 2)
    }
    if (STAG && grp == 0) __builtin_amdgcn_s_barrier();          // both groups: 2 + 2*nk barriers
    {
        unsigned char* scr = reinterpret_cast<unsigned char*>(lds) + wave * (DSTAGES * DSTAGE_ELEMS * 2 / 8);   // 9 KiB
        if (!OUT_F32 && !GLN && add2d) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int m = m0 + wm * 64 + j * 16 + fr, n = n0 + wn * 64 + i * 16 + 4 * fq;
                    const float4 e = *reinterpret_cast<const float4*>(add2d + (size_t)(m % add2d_period) * N + n);
                    acc[i][j][0] += e.x; acc[i][j][1] += e.y; acc[i][j][2] += e.z; acc[i][j][3] += e.w;
                }
        }
        epilogue_coalesced<PREC, OUT_F32, GELU, 4, OUT_F32 ? 2 : 4, 4, GLN>(acc, scr, Cv, bias, (OUT_F32 || GLN) ? add2d : nullptr,
                                                                             add2d_period, N, m0 + wm * 64, n0 + wn * 64, accumulate, lane);
    }
}

// C (ET) = GELU(LayerNorm2d_64(A B^T + bias)): the 64-column groups of N are normalised independently.
// A_lo / B_lo given: split-precision product (see the kernel), C is then FP32 (its consumer splits it again).
template <int PREC>
hipError_t launch_gemm_dual_gln(const void* A, const void* B, void* C, const float* bias, const float* gamma_beta,
                                int M, int N, int K, hipStream_t s, const void* A_lo = nullptr, const void* B_lo = nullptr) {
    dim3 grid((M / DBM) * (N / DBN)), block(DTHREADS);
    if (A_lo && B_lo)
        gemm_et_dual_kernel<PREC, true, true, true, true, true><<<grid, block, 0, s>>>(
            reinterpret_cast<const uint16_t*>(A), reinterpret_cast<const uint16_t*>(B), C, bias, gamma_beta, 1, M, N, K, 0,
            reinterpret_cast<const uint16_t*>(A_lo), reinterpret_cast<const uint16_t*>(B_lo));
    else
        gemm_et_dual_kernel<PREC, false, true, true, true><<<grid, block, 0, s>>>(
            reinterpret_cast<const uint16_t*>(A), reinterpret_cast<const uint16_t*>(B), C, bias, gamma_beta, 1, M, N, K, 0);
    return hipGetLastError();
}

template <int PREC, bool STAG = true>
hipError_t launch_gemm_dual(const void* A, const void* B, void* C, const float* bias, const float* add2d, int period,
                            int M, int N, int K, bool out_f32, bool gelu, bool accumulate, hipStream_t s) {
    dim3 grid((M / DBM) * (N / DBN)), block(DTHREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    const int acc = accumulate ? 1 : 0;
    if (out_f32) {
        if (gelu) gemm_et_dual_kernel<PREC, true, true, STAG><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
        else gemm_et_dual_kernel<PREC, true, false, STAG><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
    } else {
        if (gelu) gemm_et_dual_kernel<PREC, false, true, STAG><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
        else gemm_et_dual_kernel<PREC, false, false, STAG><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t gemm_fam::dual(int prec, bool stag, const void* A, const void* B, void* C, const float* bias, const float* add2d, int period,
                          int M, int N, int K, bool out_f32, bool gelu, bool accumulate, hipStream_t s) {
    return with_prec(prec, [&](auto P) -> hipError_t {
        if (stag) return launch_gemm_dual<P.value>(A, B, C, bias, add2d, period, M, N, K, out_f32, gelu, accumulate, s);
        return launch_gemm_dual<P.value, false>(A, B, C, bias, add2d, period, M, N, K, out_f32, gelu, accumulate, s);
    });
}

hipError_t launch_gemm_et_gln(int prec, const void* A, const void* B, void* C, const float* bias, const float* gamma_beta,
                              int M, int N, int K, hipStream_t s, const void* A_lo, const void* B_lo) {
    if (M % DBM || N % DBN || K % DBK || M <= 0 || !gamma_beta || ((A_lo == nullptr) != (B_lo == nullptr))) return hipErrorInvalidValue;
    return with_prec(prec, [&](auto P) { return launch_gemm_dual_gln<P.value>(A, B, C, bias, gamma_beta, M, N, K, s, A_lo, B_lo); });
}
