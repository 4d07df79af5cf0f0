// gemm_ring.hip -- the two gemm_et kernels with 64-wide K tiles that any valid shape can fall back on (what gemm_et computes:
// gemm.hip): gemm_et_kernel (128x128, double buffer: the v1 structure described in gemm.hip's header) and gemm_et_stag_kernel
// (256x128, three-stage LDS-DMA ring, staggered wave groups).
#include "gemm_device.h"
#include "gemm_families.h"

namespace {

constexpr int GEMM_THREADS = 256;      // BM / BN / BK and the other tile shapes the selection rule reads: gemm_select.h

// physical 16-byte chunk of logical chunk c in row r of a [rows][64] ET tile
__device__ __forceinline__ int swz(int r, int c) { return c ^ ((r >> 1) & 7); }

// LDS-DMA helper: 16 bytes per lane, global (per-lane address) -> LDS (wave-uniform base + lane*16).
__device__ __forceinline__ void glds16(const uint16_t* gsrc, uint16_t* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

template <int PREC, bool OUT_F32, bool GELU, bool GLDS, int GROUP_M>
__global__ __launch_bounds__(GEMM_THREADS) void gemm_et_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, void* __restrict__ Cv,
    const float* __restrict__ bias, const float* __restrict__ add2d, int add2d_period,
    int M, int N, int K, int accumulate) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[2][2][BM * BK];  // [buf][A|B] 64 KiB

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    // Tile order.  (1) xcd_remap gives every XCD a contiguous range of logical ids (blocks that
    // run together share one 4 MB L2).  (2) Inside that range ids walk GROUP_M tile rows fastest,
    // then tile columns: the ~64 blocks resident on an XCD form a ~8x8 super-tile, so each A and B
    // panel fetched into L2 is reused 8 times instead of streaming the whole weight matrix through
    // L2 once per tile row.
    const int tiles_n = N / BN, tiles_m = M / BM;
    const int nwg = gridDim.x;
    const int bid = xcd_remap(blockIdx.x, nwg);
    int tile_m, tile_n;
    if (GROUP_M > 1) {
        const int per_group = GROUP_M * tiles_n;
        const int group = bid / per_group, first_m = group * GROUP_M;
        const int gsz = (tiles_m - first_m) < GROUP_M ? (tiles_m - first_m) : GROUP_M;
        const int in_g = bid - group * per_group;
        tile_m = first_m + in_g % gsz;
        tile_n = in_g / gsz;
    } else {
        tile_m = bid / tiles_n;
        tile_n = bid % tiles_n;
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    // --- staging map: thread t moves chunks (row = (t>>3) + 32*i, chunk = t&7), i = 0..3 ---
    const int ld_row = tid >> 3;
    const int ld_chunk = tid & 7;
    const uint16_t* gA = A + (size_t)(m0 + ld_row) * K + ld_chunk * 8;
    const uint16_t* gB = B + (size_t)(n0 + ld_row) * K + ld_chunk * 8;

    // Staging registers.  Plain macros (not lambdas / conditionals): anything that makes the
    // compiler see these arrays through a pointer puts them in scratch.
    uint4 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;
#define GEMM_LOAD_TILE(kt_)                                                                   \
    do {                                                                                       \
        const size_t koff_ = (size_t)(kt_) * BK;                                               \
        ra0 = *reinterpret_cast<const uint4*>(gA + koff_);                                     \
        ra1 = *reinterpret_cast<const uint4*>(gA + (size_t)32 * K + koff_);                    \
        ra2 = *reinterpret_cast<const uint4*>(gA + (size_t)64 * K + koff_);                    \
        ra3 = *reinterpret_cast<const uint4*>(gA + (size_t)96 * K + koff_);                    \
        rb0 = *reinterpret_cast<const uint4*>(gB + koff_);                                     \
        rb1 = *reinterpret_cast<const uint4*>(gB + (size_t)32 * K + koff_);                    \
        rb2 = *reinterpret_cast<const uint4*>(gB + (size_t)64 * K + koff_);                    \
        rb3 = *reinterpret_cast<const uint4*>(gB + (size_t)96 * K + koff_);                    \
    } while (0)
    // swz(r + 32*i, c) == swz(r, c) ^ ... is NOT row-invariant, so compute the 4 offsets once.
    int st_off[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = ld_row + 32 * i;
        st_off[i] = r * BK + swz(r, ld_chunk) * 8;
    }
#define GEMM_STORE_TILE(buf_)                                                                 \
    do {                                                                                       \
        uint16_t* la_ = &lds[buf_][0][0];                                                      \
        uint16_t* lb_ = &lds[buf_][1][0];                                                      \
        *reinterpret_cast<uint4*>(la_ + st_off[0]) = ra0;                                      \
        *reinterpret_cast<uint4*>(la_ + st_off[1]) = ra1;                                      \
        *reinterpret_cast<uint4*>(la_ + st_off[2]) = ra2;                                      \
        *reinterpret_cast<uint4*>(la_ + st_off[3]) = ra3;                                      \
        *reinterpret_cast<uint4*>(lb_ + st_off[0]) = rb0;                                      \
        *reinterpret_cast<uint4*>(lb_ + st_off[1]) = rb1;                                      \
        *reinterpret_cast<uint4*>(lb_ + st_off[2]) = rb2;                                      \
        *reinterpret_cast<uint4*>(lb_ + st_off[3]) = rb3;                                      \
    } while (0)

    f32x4_t acc[4][4];  // [n-tile i][m-tile j]; D[i_local = n][j_local = m]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nk = K / BK;
    // GLDS staging (cdna_hip_programming.md section 5, rule 21): the DMA writes LDS linearly
    // (wave-uniform base + lane*16 B), so wave w's i-th instruction fills rows 32i + 8w .. +7
    // (lane l -> row +(l>>3), physical chunk l&7) and the swizzle goes on the SOURCE address:
    // the lane fetches logical chunk (l&7) ^ swz(row).  swz(row) does not depend on i.
    const int g_row = 8 * wave + (lane >> 3);
    const int g_chunk = (lane & 7) ^ ((g_row >> 1) & 7);
    const uint16_t* gAg = A + (size_t)(m0 + g_row) * K + g_chunk * 8;
    const uint16_t* gBg = B + (size_t)(n0 + g_row) * K + g_chunk * 8;
#define GEMM_GLDS_TILE(kt_, buf_)                                                              \
    do {                                                                                       \
        const size_t koff_ = (size_t)(kt_) * BK;                                               \
        _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                     \
            glds16(gAg + (size_t)(32 * i_) * K + koff_, &lds[buf_][0][(32 * i_ + 8 * wave) * BK]); \
            glds16(gBg + (size_t)(32 * i_) * K + koff_, &lds[buf_][1][(32 * i_ + 8 * wave) * BK]); \
        }                                                                                      \
    } while (0)

    if (GLDS) {
        GEMM_GLDS_TILE(0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        GEMM_LOAD_TILE(0);
        GEMM_STORE_TILE(0);
    }
    __syncthreads();

    const int fr = lane & 15;   // fragment row within a 16-row tile
    const int fq = lane >> 4;   // k-quarter (8 elements) within a 32-wide k-substep

    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (GLDS) {
            if (kt + 1 < nk) GEMM_GLDS_TILE(kt + 1, buf ^ 1);
        } else {
            // unconditional prefetch (the last iteration re-reads the last tile; nobody consumes it)
            GEMM_LOAD_TILE(kt + 1 < nk ? kt + 1 : kt);
        }

        const uint16_t* la = &lds[buf][0][0];
        const uint16_t* lb = &lds[buf][1][0];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            uint4 fa[4], fb[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = wm * 64 + j * 16 + fr;
                fa[j] = *reinterpret_cast<const uint4*>(la + r * BK + swz(r, ks * 4 + fq) * 8);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = wn * 64 + i * 16 + fr;
                fb[i] = *reinterpret_cast<const uint4*>(lb + r * BK + swz(r, ks * 4 + fq) * 8);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = ET<PREC>::mfma16(fb[i], fa[j], acc[i][j]);
        }

        if (GLDS) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // next tile has landed in LDS
        } else {
            GEMM_STORE_TILE(buf ^ 1);
        }
        __syncthreads();
    }

    // --- epilogue: lane holds C[m][n..n+3], m = m0 + wm*64 + j*16 + (lane&15),
    //                                      n = n0 + wn*64 + i*16 + 4*(lane>>4)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + wn * 64 + i * 16 + 4 * fq;
        float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (bias) bv = *reinterpret_cast<const float4*>(bias + n);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = m0 + wm * 64 + j * 16 + fr;
            float v0 = acc[i][j][0] + bv.x, v1 = acc[i][j][1] + bv.y;
            float v2 = acc[i][j][2] + bv.z, v3 = acc[i][j][3] + bv.w;
            if (add2d) {
                const float4 e = *reinterpret_cast<const float4*>(
                    add2d + (size_t)(m % add2d_period) * N + n);
                v0 += e.x; v1 += e.y; v2 += e.z; v3 += e.w;
            }
            if (GELU) { const float2_t g01 = gelu_erf2(float2_t{v0, v1}), g23 = gelu_erf2(float2_t{v2, v3}); v0 = g01.x; v1 = g01.y; v2 = g23.x; v3 = g23.y; }
            if (OUT_F32) {
                float* C = reinterpret_cast<float*>(Cv) + (size_t)m * N + n;
                if (accumulate) {
                    const float4 o = *reinterpret_cast<const float4*>(C);
                    v0 += o.x; v1 += o.y; v2 += o.z; v3 += o.w;
                }
                *reinterpret_cast<float4*>(C) = make_float4(v0, v1, v2, v3);
            } else {
                uint16_t* C = reinterpret_cast<uint16_t*>(Cv) + (size_t)m * N + n;
                uint2 o;
                o.x = pack2<PREC>(v0, v1);
                o.y = pack2<PREC>(v2, v3);
                *reinterpret_cast<uint2*>(C) = o;
            }
        }
    }
}

template <int PREC, bool GLDS, int GROUP_M>
hipError_t launch_gemm_prec(const void* A, const void* B, void* C, const float* bias,
                            const float* add2d, int period, int M, int N, int K, bool out_f32,
                            bool gelu, bool accumulate, hipStream_t s) {
    dim3 grid((M / BM) * (N / BN)), block(GEMM_THREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    const int acc = accumulate ? 1 : 0;
    if (out_f32) {
        if (gelu)
            gemm_et_kernel<PREC, true, true, GLDS, GROUP_M><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
        else
            gemm_et_kernel<PREC, true, false, GLDS, GROUP_M><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
    } else {
        if (gelu)
            gemm_et_kernel<PREC, false, true, GLDS, GROUP_M><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
        else
            gemm_et_kernel<PREC, false, false, GLDS, GROUP_M><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Shared geometry of the 256x128x64 staggered kernel below (its lock-step round-1 flavour was removed): block tile, 512 threads = 8 waves (4 along M x 2 along N, each
// a 64x64 sub-tile exactly as above), THREE-stage LDS ring filled by LDS-DMA with a COUNTED
// s_waitcnt vmcnt: the loads of tile t+2 are issued before computing tile t and only tile t+1 is
// waited for at the (raw) barrier, so DMA traffic stays in flight across barriers instead of
// draining every K step (rocprofv3 on the 2-stage kernel: 47 % of wave cycles parked in
// s_waitcnt/s_barrier, MFMA busy 30 %).  144 KiB LDS -> one block (8 waves) per CU.
// ---------------------------------------------------------------------------------------------
constexpr int PBN = 128, PTHREADS = 512, PSTAGES = 3;
constexpr int PSTAGE_ELEMS = (PBM + PBN) * BK;          // A rows then B rows, 64 ET each
constexpr int P_GLDS_PER_TILE = (PBM + PBN) * BK * 2 / (PTHREADS * 16);   // 6 per thread

// one K tile (A: 4 x 64 rows, B: 2 x 64 rows) into ring stage `stage_`: six DMA pieces per wave
#define PIPE_ISSUE(kt_, stage_)                                                                 \
    do {                                                                                         \
        const size_t koff_ = (size_t)(kt_) * BK;                                                 \
        constexpr int SB_ = (stage_) * PSTAGE_ELEMS * 2;                                         \
        glds16_asm<SB_ + 0 * 64 * BK * 2>(gAg + koff_, wave_lds_base);                           \
        glds16_asm<SB_ + 1 * 64 * BK * 2>(gAg + rs64 + koff_, wave_lds_base);                    \
        glds16_asm<SB_ + 2 * 64 * BK * 2>(gAg + 2 * rs64 + koff_, wave_lds_base);                \
        glds16_asm<SB_ + 3 * 64 * BK * 2>(gAg + 3 * rs64 + koff_, wave_lds_base);                \
        glds16_asm<SB_ + PBM * BK * 2 + 0 * 64 * BK * 2>(gBg + koff_, wave_lds_base);            \
        glds16_asm<SB_ + PBM * BK * 2 + 1 * 64 * BK * 2>(gBg + rs64 + koff_, wave_lds_base);     \
    } while (0)

// ---------------------------------------------------------------------------------------------
// gemm_et_stag_kernel: the tile / ring / DMA described above, and the two waves that share
// a SIMD (waves w and w+4) run STAGGERED by one barrier interval.  Every K step is cut into four
// segments separated by raw barriers -- L0 (fragment reads, k 0..31 + DMA issue), C0 (16 MFMAs),
// L1 (reads, k 32..63), C1 (16 MFMAs) -- and group 1 (waves 4..7) executes one extra barrier up
// front, so while group 0 is in a C segment group 1 is in an L segment and vice versa: the matrix
// pipe of every SIMD always has one wave feeding it while its partner waits on LDS (rocprofv3 on the
// lock-step kernel: 48 % of wave cycles parked, MFMA busy 37 %).  s_setprio(1) around the MFMA
// segments lets the computing wave win issue arbitration (cdna_hip_programming.md T5).
//
// Ring safety with the stagger (interval numbering 4*kt + {0,1,2,3} for group 0, +1 for group 1):
//  WAR  the slot of tile kt-1 is last read by group 1 in interval 4kt-1; its refill (tile kt+2) is
//       issued in an L0 segment, i.e. interval 4kt (group 0) / 4kt+1 (group 1): after that barrier.
//  RAW  tile kt+1 is first read in interval 4kt+4; every wave waits vmcnt for its own share at the
//       end of BOTH its L1 and C1 segments (interval 4kt+3 for either group) and then passes the
//       barrier that opens interval 4kt+4.
// Both groups execute exactly 2 + 4*nk barriers.
// ---------------------------------------------------------------------------------------------
template <int PREC, bool OUT_F32, bool GELU>
__global__ __launch_bounds__(PTHREADS) void gemm_et_stag_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, void* __restrict__ Cv,
    const float* __restrict__ bias, const float* __restrict__ add2d, int add2d_period,
    int M, int N, int K, int accumulate) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[PSTAGES * PSTAGE_ELEMS];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform
    const int grp = wave >> 2;
    const int wm = wave >> 1, wn = wave & 1;

    constexpr int GROUP = 8;
    const int tiles_n = N / PBN, tiles_m = M / PBM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int per_group = GROUP * tiles_n;
    const int group = bid / per_group, first_m = group * GROUP;
    const int gsz = (tiles_m - first_m) < GROUP ? (tiles_m - first_m) : GROUP;
    const int in_g = bid - group * per_group;
    const int tile_m = first_m + in_g % gsz, tile_n = in_g / gsz;
    const int m0 = tile_m * PBM, n0 = tile_n * PBN;

    const int g_row = 8 * wave + (lane >> 3);
    const int g_chunk = (lane & 7) ^ ((g_row >> 1) & 7);
    const uint16_t* gAg = A + (size_t)(m0 + g_row) * K + g_chunk * 8;
    const uint16_t* gBg = B + (size_t)(n0 + g_row) * K + g_chunk * 8;
    const uint32_t wave_lds_base = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds + (uint32_t)wave * (8 * BK * 2));
    const size_t rs64 = (size_t)64 * K;

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nk = K / BK;
    PIPE_ISSUE(0, 0);
    if (nk > 1) {
        PIPE_ISSUE(1, 1);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P_GLDS_PER_TILE) : "memory");
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    if (grp == 1) __builtin_amdgcn_s_barrier();          // stagger: group 1 runs one interval behind

    const int fr = lane & 15, fq = lane >> 4;
#define STAG_LOAD(S_, KS_)                                                                        \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                               \
        const int r = wm * 64 + j * 16 + fr;                                                      \
        fa[j] = *reinterpret_cast<const uint4*>(lds + (S_) * PSTAGE_ELEMS + r * BK + swz(r, (KS_) * 4 + fq) * 8); \
    }                                                                                             \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                               \
        const int r = wn * 64 + i * 16 + fr;                                                      \
        fb[i] = *reinterpret_cast<const uint4*>(lds + (S_) * PSTAGE_ELEMS + PBM * BK + r * BK + swz(r, (KS_) * 4 + fq) * 8); \
    }
#define STAG_MMA()                                                                                \
    __builtin_amdgcn_s_setprio(1);                                                                \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                 \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) acc[i][j] = ET<PREC>::mfma16(fb[i], fa[j], acc[i][j]); \
    __builtin_amdgcn_s_setprio(0);
#define STAG_WAIT_NEXT(kt_)                                                                       \
    if ((kt_) + 2 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(P_GLDS_PER_TILE) : "memory");    \
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#define STAG_STEP(kt_, S_)                                                                        \
    if ((kt_) < nk) {                                                                             \
        uint4 fa[4], fb[4];                                                                       \
        /* L0 */                                                                                  \
        if ((kt_) + 2 < nk) PIPE_ISSUE((kt_) + 2, ((S_) + 2) % PSTAGES);                          \
        STAG_LOAD(S_, 0)                                                                          \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                        \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        __builtin_amdgcn_s_barrier();                                                             \
        /* C0 */                                                                                  \
        STAG_MMA()                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        __builtin_amdgcn_s_barrier();                                                             \
        /* L1 */                                                                                  \
        STAG_LOAD(S_, 1)                                                                          \
        STAG_WAIT_NEXT(kt_)                                                                       \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                        \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        __builtin_amdgcn_s_barrier();                                                             \
        /* C1 */                                                                                  \
        STAG_MMA()                                                                                \
        STAG_WAIT_NEXT(kt_)                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        __builtin_amdgcn_s_barrier();                                                             \
    }
    for (int kt = 0; kt < nk; kt += PSTAGES) {
        STAG_STEP(kt, 0)
        STAG_STEP(kt + 1, 1)
        STAG_STEP(kt + 2, 2)
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();          // group 0 finishes one interval early
    // every wave is past its last ring read here -> the ring is free scratch (18 KiB per wave)
    {
        unsigned char* scr = reinterpret_cast<unsigned char*>(lds) + wave * (PSTAGES * PSTAGE_ELEMS * 2 / 8);
        // add2d (if any) only comes with fp32 output in the engine; ET output ignores accumulate
        if (!OUT_F32 && add2d) {
            // rare combination (ET out + 2-D addend): fold the addend in before the bounce
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int m = m0 + wm * 64 + j * 16 + fr, n = n0 + wn * 64 + i * 16 + 4 * fq;
                    const float4 e = *reinterpret_cast<const float4*>(add2d + (size_t)(m % add2d_period) * N + n);
                    acc[i][j][0] += e.x; acc[i][j][1] += e.y; acc[i][j][2] += e.z; acc[i][j][3] += e.w;
                }
        }
        epilogue_coalesced<PREC, OUT_F32, GELU, 4, 4>(acc, scr, Cv, bias, OUT_F32 ? add2d : nullptr, add2d_period, N,
                                                      m0 + wm * 64, n0 + wn * 64, accumulate, lane);
    }
}

template <int PREC>
hipError_t launch_gemm_stag(const void* A, const void* B, void* C, const float* bias, const float* add2d, int period,
                            int M, int N, int K, bool out_f32, bool gelu, bool accumulate, hipStream_t s) {
    dim3 grid((M / PBM) * (N / PBN)), block(PTHREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    const int acc = accumulate ? 1 : 0;
    if (out_f32) {
        if (gelu) gemm_et_stag_kernel<PREC, true, true><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
        else gemm_et_stag_kernel<PREC, true, false><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
    } else {
        if (gelu) gemm_et_stag_kernel<PREC, false, true><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
        else gemm_et_stag_kernel<PREC, false, false><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
    }
    return hipGetLastError();
}

}  // namespace

namespace gemm_fam {

hipError_t base(int prec, bool glds, int group_m, const void* A, const void* B, void* C, const float* bias, const float* add2d, int period,
                int M, int N, int K, bool out_f32, bool gelu, bool accumulate, hipStream_t s) {
    return with_prec(prec, [&](auto P) -> hipError_t {
        auto go = [&](auto GLDS, auto GROUP_M) {
            return launch_gemm_prec<P.value, (GLDS.value != 0), GROUP_M.value>(A, B, C, bias, add2d, period, M, N, K, out_f32, gelu, accumulate, s);
        };
        if (glds) return group_m == 1 ? go(Int<1>{}, Int<1>{}) : go(Int<1>{}, Int<8>{});
        return group_m == 1 ? go(Int<0>{}, Int<1>{}) : go(Int<0>{}, Int<8>{});
    });
}

hipError_t stag(int prec, const void* A, const void* B, void* C, const float* bias, const float* add2d, int period,
                int M, int N, int K, bool out_f32, bool gelu, bool accumulate, hipStream_t s) {
    return with_prec(prec, [&](auto P) { return launch_gemm_stag<P.value>(A, B, C, bias, add2d, period, M, N, K, out_f32, gelu, accumulate, s); });
}

}  // namespace gemm_fam
