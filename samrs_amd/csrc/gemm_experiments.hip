// gemm_experiments.hip -- the GEMM kernels that were measured and NOT adopted, kept as the lab record with their tests: the round-2
// 32x32x16 kernels gemm_et_m32_kernel and gemm_et_w4_kernel and the LayerNorm fold built on them (launch_gemm_et_stats,
// launch_gemm_et_fold).  make EXPERIMENTS=1 builds them (tools / A-B runs); the product build has the two refusing stubs alone.
// The timing ablations of the live main loops and the fold's consumer flavour sit with their kernels (gemm.hip).
#include "gemm_device.h"
#include "gemm_families.h"

#ifndef SAMRS_EXPERIMENTS
hipError_t launch_gemm_et_stats(int, const void*, const void*, float*, const float*, void*, float*, int, int, int, hipStream_t) { return hipErrorInvalidValue; }
hipError_t launch_gemm_et_fold(int, const void*, const void*, void*, const float*, const float*, const float*, int, int, int, bool, hipStream_t) { return hipErrorInvalidValue; }
#else
namespace {

// ---------------------------------------------------------------------------------------------
// gemm_et_m32_kernel: the pair-stage 256x320 kernel (same LDS image, same whole-line LDS-DMA map) on
// v_mfma_f32_32x32x16 with a SYMMETRIC, register-double-buffered schedule.
//
// Why another main loop.  Measured on the 16x16x32 kernels above: a 64-k stage takes ~3.5 k cycles
// against 2.56 k of matrix-pipe time; one 16x16x32 MFMA occupies the pipe for ~17 cycles (MI355X_MICROARCH.md: 4.2
// quad-cycles, i.e. 6 % above its nominal 16), leaves ~4 issue slots before the next one is due, and an LDS-DMA piece
// (m0 write + s_nop + the load + address SALU) does not fit into such a gap -- every piece opens a bubble in the issuing
// wave's MFMA stream that only the partner wave can fill, which is why that schedule needs the two wave groups half a
// stage apart and L / C segments.  A 32x32x16 MFMA runs 32 cycles at the full rate, reads HALF the operand registers
// per FLOP (2 x 512 elements for 32 K FLOP instead of 16 K) and leaves ~8 issue slots: one ds_read_b128 plus one DMA
// piece fit behind every MFMA.  So here every wave runs ONE uninterrupted MFMA stream; the fragments of k-step s+1 are
// read while the MFMAs of step s run (two register sets), the DMA pieces ride in the same gaps, and there is no load
// segment and no group asymmetry.  The two waves of a SIMD share its matrix pipe by the hardware's age arbitration.
//
// Wave layout 4 (M) x 2 (N): wave tile 64 x 160 = 2 x 5 MFMA tiles, 160 accumulator registers; a wave owns whole
// 320-byte (f16) / 640-byte (fp32) row segments of the output, so the epilogue bounces through a wave-private scratch
// without block barriers.  Per 16-k step and wave: 10 MFMAs, 7 ds_read_b128 (14.3 KiB per 32 k against 13.3 KiB for
// the 128 x 80 wave tile).
//
// Stage hand-over (one block barrier per 64-k stage, placed between steps 2 and 3 of the stage):
//     steps 0, 1, 2 of stage t : MFMAs | reads of the next step's fragments (buffer t & 1)
//     lgkmcnt(0) (every fragment of stage t is in registers), vmcnt(0) (this wave's pieces of stage t+1 have landed), barrier B_t
//     step 3 of stage t        : MFMAs | reads of step 0 of stage t+1 (other buffer) | DMA pieces of stage t+2 -> buffer t & 1
// so a stage is in flight for three steps (~2 k cycles).  Persistent: the stream of stages simply continues into the next
// tile -- at t = nst-2 the pieces issued are the next tile's stage 0 (they land under the last stage and the epilogue);
// the epilogue bounces through buffer 1 (free after B_nst-1; nst must be even), and the next tile's stage 1 goes out
// right after it.  K % 128 == 0, M % 256 == 0, N % 320 == 0, no 2-D addend.
// k is accumulated in 16-wide MFMA steps, so results are NOT bit-identical with the 16x16x32 kernels (same fp32
// accumulation error class; tests/test_kernels_gpu.py::test_gemm_m32_*).
// ---------------------------------------------------------------------------------------------
constexpr int M32_RS = 144;                   // scratch row stride (bytes): 128 data bytes + 16; 36 words = 4 (mod 32)

// Epilogue of one wave tile: acc[i][j] = 32 (n) x 32 (m) block, lane (m = l & 31, h = l >> 5) holds n = 8 g + 4 h + 0..3
// for g = 0..3 in registers 4 g .. 4 g + 3.  Bounce through `scr` (wave-private, 32 rows x M32_RS bytes) so that the global
// accesses are whole 128-byte row segments, 8 rows per instruction.
// STATS (fp32 output = the residual stream; the LayerNorm that follows is folded into the next GEMM, gemm_et_x64p_kernel<FOLD>):
// besides C the final values are written rounded to ET into Xh (same [M][N] shape), and stats[m][n_base / 160] receives
// (mean, M2 = sum of squared deviations) of the wave's 160 columns of row m.  In the read-out a row's 32 columns of a pass sit
// in 8 consecutive lanes: group mean / M2 by three xor-shuffles each (two-pass inside the group), merged into the running
// pair over the five passes by Chan's update -- no E[x^2] - mean^2 cancellation, fixed order, bit-reproducible.
template <int PREC, bool OUT_F32, bool GELU, bool STATS = false, int NJ = 2>
__device__ __forceinline__ void epilogue_m32(f32x16_t (&acc)[5][NJ], unsigned char* scr, void* __restrict__ Cv,
                                             const float* __restrict__ bias, int N, int m_base, int n_base, int wn,
                                             int accumulate, int lane, uint16_t* __restrict__ Xh = nullptr,
                                             float2* __restrict__ stats = nullptr) {
    const int l31 = lane & 31, h = lane >> 5;
    if constexpr (OUT_F32) {
        float* C = reinterpret_cast<float*>(Cv);
        bool first = true;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float rmean[4], rm2[4];
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                // the residual (old C) does not depend on the accumulators: its loads go out first
                float4 res[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int idx = lane + 64 * p, row = idx >> 3, ch = idx & 7;
                    res[p] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (accumulate) res[p] = *reinterpret_cast<const float4*>(C + (size_t)(m_base + j * 32 + row) * N + n_base + i * 32 + ch * 4);
                }
                if (!first) wave_lds_sync_g();
                first = false;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 bv = bias ? *reinterpret_cast<const float4*>(bias + n_base + i * 32 + 8 * g + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f);
                    float v0 = acc[i][j][4 * g] + bv.x, v1 = acc[i][j][4 * g + 1] + bv.y;
                    float v2 = acc[i][j][4 * g + 2] + bv.z, v3 = acc[i][j][4 * g + 3] + bv.w;
                    if (GELU) { const float2_t g01 = gelu_erf2(float2_t{v0, v1}), g23 = gelu_erf2(float2_t{v2, v3}); v0 = g01.x; v1 = g01.y; v2 = g23.x; v3 = g23.y; }
                    *reinterpret_cast<float4*>(scr + l31 * M32_RS + (8 * g + 4 * h) * 4) = make_float4(v0, v1, v2, v3);
                }
                wave_lds_sync_g();
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int idx = lane + 64 * p, row = idx >> 3, ch = idx & 7;
                    float4 v = *reinterpret_cast<const float4*>(scr + row * M32_RS + ch * 16);
                    v.x += res[p].x; v.y += res[p].y; v.z += res[p].z; v.w += res[p].w;
                    const size_t o = (size_t)(m_base + j * 32 + row) * N + n_base + i * 32 + ch * 4;
                    *reinterpret_cast<float4*>(C + o) = v;
                    if constexpr (STATS) {
                        uint2 e;
                        e.x = pack2<PREC>(v.x, v.y);
                        e.y = pack2<PREC>(v.z, v.w);
                        *reinterpret_cast<uint2*>(Xh + o) = e;
                        float sm = (v.x + v.y) + (v.z + v.w);
                        sm += __shfl_xor(sm, 1, 64); sm += __shfl_xor(sm, 2, 64); sm += __shfl_xor(sm, 4, 64);
                        const float gm = sm * (1.0f / 32.0f);
                        const float d0 = v.x - gm, d1 = v.y - gm, d2 = v.z - gm, d3 = v.w - gm;
                        float gq = (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
                        gq += __shfl_xor(gq, 1, 64); gq += __shfl_xor(gq, 2, 64); gq += __shfl_xor(gq, 4, 64);
                        if (i == 0) { rmean[p] = gm; rm2[p] = gq; }
                        else {
                            const float d = gm - rmean[p];
                            rmean[p] += d * (1.0f / (i + 1));
                            rm2[p] += gq + d * d * (32.0f * i / (i + 1));
                        }
                    }
                }
            }
            if constexpr (STATS) {
                if ((lane & 7) == 0) {
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        stats[(size_t)(m_base + j * 32 + (lane >> 3) + 8 * p) * (N / 160) + n_base / 160] = make_float2(rmean[p], rm2[p]);
                }
            }
        }
    } else {
        uint16_t* C = reinterpret_cast<uint16_t*>(Cv);
        // one pass = n-tiles [I0, I0 + CNT): CNT * 64 bytes per row.  The wave's 320-byte row segment starts on a 128-byte
        // line for wn = 0 and in the middle of one for wn = 1, so the passes are grouped {0,1}{2,3}{4} / {0}{1,2}{3,4}: every
        // two-tile pass writes whole lines.
#define M32_ET_PASS(j_, I0, CNT)                                                                                     \
        do {                                                                                                         \
            wave_lds_sync_g();                                                                                       \
            _Pragma("unroll") for (int ii = 0; ii < (CNT); ++ii)                                                     \
            _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                          \
                const int i = (I0) + ii;                                                                             \
                const float4 bv = bias ? *reinterpret_cast<const float4*>(bias + n_base + i * 32 + 8 * g + 4 * h) : make_float4(0.f, 0.f, 0.f, 0.f); \
                float v0 = acc[i][j_][4 * g] + bv.x, v1 = acc[i][j_][4 * g + 1] + bv.y;                              \
                float v2 = acc[i][j_][4 * g + 2] + bv.z, v3 = acc[i][j_][4 * g + 3] + bv.w;                          \
                if (GELU) { const float2_t g01 = gelu_erf2(float2_t{v0, v1}), g23 = gelu_erf2(float2_t{v2, v3}); v0 = g01.x; v1 = g01.y; v2 = g23.x; v3 = g23.y; } \
                uint2 o;                                                                                             \
                o.x = pack2<PREC>(v0, v1);                                                                           \
                o.y = pack2<PREC>(v2, v3);                                                                           \
                *reinterpret_cast<uint2*>(scr + l31 * M32_RS + (ii * 32 + 8 * g + 4 * h) * 2) = o;                   \
            }                                                                                                        \
            wave_lds_sync_g();                                                                                       \
            _Pragma("unroll") for (int p = 0; p < 2 * (CNT); ++p) {                                                  \
                const int idx = lane + 64 * p, row = idx / (4 * (CNT)), ch = idx % (4 * (CNT));                      \
                const uint4 v = *reinterpret_cast<const uint4*>(scr + row * M32_RS + ch * 16);                       \
                *reinterpret_cast<uint4*>(C + (size_t)(m_base + (j_) * 32 + row) * N + n_base + (I0) * 32 + ch * 8) = v; \
            }                                                                                                        \
        } while (0)
        if (wn == 0) {
#pragma unroll
            for (int j = 0; j < NJ; ++j) { M32_ET_PASS(j, 0, 2); M32_ET_PASS(j, 2, 2); M32_ET_PASS(j, 4, 1); }
        } else {
#pragma unroll
            for (int j = 0; j < NJ; ++j) { M32_ET_PASS(j, 0, 1); M32_ET_PASS(j, 1, 2); M32_ET_PASS(j, 3, 2); }
        }
#undef M32_ET_PASS
    }
}

// SPREAD: 0 = the 9 DMA pieces of a stage all go out in step 3 (one behind each of the first 9 MFMAs); 1 = pieces 0-4 in
// step 3 and pieces 5-8 in step 0 of the following stage (fewer fillers per gap, one step less in flight)
template <int PREC, bool OUT_F32, bool GELU, int SPREAD, bool STATS = false>
__global__ __launch_bounds__(QTHREADS) void gemm_et_m32_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, void* __restrict__ Cv,
    const float* __restrict__ bias, int M, int N, int K, int accumulate,
    uint16_t* __restrict__ Xh = nullptr, float2* __restrict__ stats = nullptr) {
    static_assert(!STATS || (OUT_F32 && !GELU), "row statistics accompany the fp32 residual output only");
    constexpr int NI = 5, NJ = 2;
    constexpr int XBN = 32 * NI * 2;                       // 320
    constexpr int XROWS = QBM + XBN;
    constexpr int XSTAGE_ELEMS = XROWS * XBK;
    constexpr uint32_t XSB = XSTAGE_ELEMS * 2;             // 72 KiB per stage
    constexpr int NP3 = SPREAD ? 5 : 9;                    // pieces [0, NP3) ride in step 3, [NP3, 9) in the next step 0
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * XSTAGE_ELEMS];   // 144 KiB, ONE object

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;   // wave tile rows wm*64.., cols wn*160..

    constexpr int GROUP = 8;
    const int tiles_n = N / XBN, tiles_m = M / QBM, ntiles = tiles_n * tiles_m;
    const int per_group = GROUP * tiles_n;
#define M32_TILE(L_, m_, n_)                                                                     \
    do {                                                                                         \
        const int bid_ = xcd_remap((L_), ntiles);                                                \
        const int group_ = bid_ / per_group, first_m_ = group_ * GROUP;                           \
        const int gsz_ = (tiles_m - first_m_) < GROUP ? (tiles_m - first_m_) : GROUP;            \
        const int in_g_ = bid_ - group_ * per_group;                                             \
        (m_) = (first_m_ + in_g_ % gsz_) * QBM;                                                  \
        (n_) = (in_g_ / gsz_) * XBN;                                                             \
    } while (0)

    // DMA map: identical to the 16x16x32 pair-stage kernels (piece q of a wave = stage rows 64 q + 8 wave .. + 7)
    const int prow = 8 * wave + ((lane >> 2) & 7);
    const uint32_t voff = ((uint32_t)prow * (uint32_t)K + (uint32_t)(lane >> 5) * 32u + (uint32_t)qswz(prow, lane & 3) * 8u) * 2u;
    const size_t rs64 = (size_t)64 * K;
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds + (uint32_t)wave * 1024u);
    // piece q_ (literal) of the stage whose A / B rows start at pa_ / pb_ (wave-uniform) into the buffer at byte offset wr_
#define M32_PIECE(pa_, pb_, wr_, q_)                                                                       \
    glds16_m(voff, ((q_) < 4 ? (pa_) + (size_t)(q_) * rs64 : (pb_) + (size_t)((q_) - 4) * rs64),          \
             lds0 + (wr_) + ((q_) < 4 ? (q_) * 8192u : (uint32_t)(QBM * XBK * 2) + ((q_) - 4) * 8192u))

    // fragment BYTE offsets inside a stage for k-step 0 of k-half 0 (16-byte chunk h of the row); step parity 1 = chunk
    // h + 2 = the physical chunk XOR 2 (byte offset XOR 32), k-half 1 = +512
    const int nst = K / XBK;
    const int l31 = lane & 31, hh = lane >> 5;
    uint32_t offA[NJ], offB[NI];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { const int r = wm * 64 + j * 32 + l31; offA[j] = ((r >> 3) * 512 + (r & 7) * 32 + qswz(r, hh) * 8) * 2; }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int r = QBM + wn * 160 + i * 32 + l31;
        offB[i] = ((r >> 3) * 512 + (r & 7) * 32 + qswz(r, hh) * 8) * 2;
    }
    const unsigned char* ldsb = reinterpret_cast<const unsigned char*>(lds);

    // fragments of k-step s_ (0..3) of the stage in the buffer at byte offset rd_ -> register set fa / fb
#define M32_RDB(fb_, rd_, s_, i_) fb_[i_] = *reinterpret_cast<const uint4*>(ldsb + (rd_) + ((s_) >> 1) * 512 + (offB[i_] ^ (((s_) & 1) * 32u)))
#define M32_RDA(fa_, rd_, s_, j_) fa_[j_] = *reinterpret_cast<const uint4*>(ldsb + (rd_) + ((s_) >> 1) * 512 + (offA[j_] ^ (((s_) & 1) * 32u)))
    // one k-step: 10 MFMAs on the set (ca_, cb_); behind MFMA k one read of the NEXT step's set (na_, nb_) from (nrd_, ns_)
    // and DMA piece Q0_ + k (while < Q1_) of the stage (pa_, pb_) -> buffer wr_: D_ = 0 none, 1 always, 2 when dma_ (wave-
    // uniform) is set.  The accumulators never sit inside a conditional region.
#define M32_SLOT(k_, i_, j_, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)             \
        acc[i_][j_] = ET<PREC>::mfma32(cb_[i_], ca_[j_], acc[i_][j_]);                                     \
        if constexpr ((k_) < 5) { M32_RDB(nb_, nrd_, ns_, ((k_) < 5 ? (k_) : 0)); }                        \
        else if constexpr ((k_) < 7) { M32_RDA(na_, nrd_, ns_, ((k_) >= 5 && (k_) < 7 ? (k_) - 5 : 0)); }  \
        if constexpr ((D_) != 0 && (Q0_) + (k_) < (Q1_)) {                                                 \
            if ((D_) == 1 || (dma_)) M32_PIECE(pa_, pb_, wr_, ((Q0_) + (k_) < 9 ? (Q0_) + (k_) : 0));      \
        }                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);
#define M32_STEP(ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                         \
        M32_SLOT(0, 0, 0, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                \
        M32_SLOT(1, 1, 0, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                \
        M32_SLOT(2, 2, 0, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                \
        M32_SLOT(3, 3, 0, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                \
        M32_SLOT(4, 4, 0, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                \
        M32_SLOT(5, 0, 1, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                \
        M32_SLOT(6, 1, 1, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                \
        M32_SLOT(7, 2, 1, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                \
        M32_SLOT(8, 3, 1, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                \
        M32_SLOT(9, 4, 1, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)
    // one 64-k stage held in buffer rd.  Step 0 carries the late pieces [NP3, 9) of the stage that goes into the OTHER buffer
    // (D0_, d0_, a0_, b0_); step 3, after the hand-over barrier, the early pieces [0, NP3) of the stage that goes into THIS
    // buffer (D3_, d3_, a3_, b3_).
#define M32_STAGE(D0_, d0_, a0_, b0_, D3_, d3_, a3_, b3_)                                                  \
        {                                                                                                  \
            const uint32_t ot = XSB - rd;                                                                  \
            M32_STEP(fa0, fb0, fa1, fb1, rd, 1, D0_, d0_, NP3, 9, a0_, b0_, ot)                            \
            M32_STEP(fa1, fb1, fa0, fb0, rd, 2, 0, false, 0, 0, a0_, b0_, ot)                              \
            M32_STEP(fa0, fb0, fa1, fb1, rd, 3, 0, false, 0, 0, a0_, b0_, ot)                              \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                    \
            __builtin_amdgcn_s_barrier();                                                                  \
            __builtin_amdgcn_sched_barrier(0);                                                             \
            M32_STEP(fa1, fb1, fa0, fb0, ot, 0, D3_, d3_, 0, NP3, a3_, b3_, rd)                            \
            rd = ot;                                                                                       \
        }

    int L = blockIdx.x, m0, n0;
    M32_TILE(L, m0, n0);
    const uint16_t* sA = A + (size_t)m0 * K;       // rows of the tile being computed (wave-uniform: SGPR pairs)
    const uint16_t* sB = B + (size_t)n0 * K;
    M32_PIECE(sA, sB, 0u, 0); M32_PIECE(sA, sB, 0u, 1); M32_PIECE(sA, sB, 0u, 2); M32_PIECE(sA, sB, 0u, 3); M32_PIECE(sA, sB, 0u, 4);
    M32_PIECE(sA, sB, 0u, 5); M32_PIECE(sA, sB, 0u, 6); M32_PIECE(sA, sB, 0u, 7); M32_PIECE(sA, sB, 0u, 8);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    f32x16_t acc[NI][NJ];
    for (;;) {
        // the tile after this one (its stage 0 is fed from inside this tile's main loop)
        const int Ln = L + (int)gridDim.x;
        const bool more = Ln < ntiles;
        int m1 = m0, n1 = n0;
        if (more) M32_TILE(Ln, m1, n1);
        const uint16_t* nA = A + (size_t)m1 * K;
        const uint16_t* nB = B + (size_t)n1 * K;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        {   // early pieces of stage 1 -> buffer 1 (the late ones ride in step 0 of stage 0)
            const uint16_t* a1 = sA + XBK;
            const uint16_t* b1 = sB + XBK;
            M32_PIECE(a1, b1, XSB, 0); M32_PIECE(a1, b1, XSB, 1); M32_PIECE(a1, b1, XSB, 2); M32_PIECE(a1, b1, XSB, 3); M32_PIECE(a1, b1, XSB, 4);
            if constexpr (!SPREAD) { M32_PIECE(a1, b1, XSB, 5); M32_PIECE(a1, b1, XSB, 6); M32_PIECE(a1, b1, XSB, 7); M32_PIECE(a1, b1, XSB, 8); }
        }
        uint4 fa0[NJ], fb0[NI], fa1[NJ], fb1[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) M32_RDB(fb0, 0u, 0, i);
#pragma unroll
        for (int j = 0; j < NJ; ++j) M32_RDA(fa0, 0u, 0, j);
        __builtin_amdgcn_sched_barrier(0);
        uint32_t rd = 0;
        // stage t: step 0 completes stage t+1, step 3 starts stage t+2
        const uint16_t* pa = sA + XBK;
        const uint16_t* pb = sB + XBK;
        for (int t = 0; t + 2 < nst; ++t) {
            M32_STAGE(1, true, pa, pb, 1, true, pa + XBK, pb + XBK)
            pa += XBK;
            pb += XBK;
        }
        // t = nst-2 (buffer 0): completes the last stage; starts the NEXT tile's stage 0 in buffer 0 when there is one
        M32_STAGE(1, true, pa, pb, 2, more, nA, nB)
        // t = nst-1 (buffer 1): completes the next tile's stage 0
        M32_STAGE(2, more, nA, nB, 0, false, nA, nB)
        // all fragment reads of this tile are complete (B_nst-1); buffer 1 held its last stage -> scratch
        {
            unsigned char* scr = reinterpret_cast<unsigned char*>(lds) + XSB + wave * (XSB / 8);
            epilogue_m32<PREC, OUT_F32, GELU, STATS>(acc, scr, Cv, bias, N, m0 + wm * 64, n0 + wn * 160, wn, accumulate, lane, Xh, stats);
        }
        if (!more) break;
        __builtin_amdgcn_s_barrier();              // every wave is done with its scratch before stage 1 of the next tile lands there
        L = Ln; m0 = m1; n0 = n1; sA = nA; sB = nB;
    }
#undef M32_TILE
#undef M32_PIECE
#undef M32_RDA
#undef M32_RDB
#undef M32_SLOT
#undef M32_STEP
#undef M32_STAGE
}

// persistent = one block per CU walks the tiles; otherwise one tile per block (same kernel: `more` is never true)
template <int PREC, int SPREAD>
hipError_t launch_gemm_m32(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, bool out_f32, bool gelu,
                           bool accumulate, bool persistent, hipStream_t s) {
    const int ntiles = (M / QBM) * (N / WBN);
    const int n_cu = cu_count();
    dim3 grid(persistent && ntiles > n_cu ? n_cu : ntiles), block(QTHREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    const int acc = accumulate ? 1 : 0;
    if (out_f32) {
        if (gelu) gemm_et_m32_kernel<PREC, true, true, SPREAD><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc);
        else gemm_et_m32_kernel<PREC, true, false, SPREAD><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc);
    } else {
        if (gelu) gemm_et_m32_kernel<PREC, false, true, SPREAD><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc);
        else gemm_et_m32_kernel<PREC, false, false, SPREAD><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// gemm_et_w4_kernel: the symmetric 32x32x16 schedule above on FOUR waves with 512 registers each (one wave per SIMD).
//
// Why: the DVFS probe says the encoder GEMMs are limited by energy per FLOP, and the one structural knob on it
// is the number of bytes that cross LDS -> registers per FLOP, i.e. the perimeter of the WAVE tile: 8 waves x (128 + 80) rows
// of fragments per k-step for the 2 x 4 layout, 8 x (64 + 160) for the 4 x 2 layout of gemm_et_m32_kernel, 4 x (128 + 160) here
// (-31 % / -36 %).  A 128 x 160 wave tile needs 320 accumulator registers; hipcc keeps all MFMA results of a kernel either in
// VGPRs or in AGPRs (256 each), so the MFMAs are issued from inline asm: the 16 accumulator tiles of n-tiles 0-3 are constrained
// to AGPRs ("+a"), the 4 tiles of n-tile 4 to VGPRs ("+v"); everything else (fragments 2 x 36, addressing) fits the VGPR half.
// The compiler does not know these statements are MFMAs, so the two hazards it would pad are padded by hand (s_nop after the
// accumulators are zeroed and before the epilogue reads them).
//
// Stage image, DMA pieces (now 18 per wave and stage: rows 32 q + 8 wave .. + 7), hand-over barrier, persistent stage stream and
// epilogue are those of gemm_et_m32_kernel; pieces 0-9 ride in step 3 (slots 10-19, the reads use slots 0-8), pieces 10-17 in
// the next step 0.  With one wave per SIMD nothing covers a stall, so the single barrier per stage costs what it costs.
// ---------------------------------------------------------------------------------------------
template <int PREC, bool AG>
__device__ __forceinline__ void mfma32_asm(f32x16_t& c, const uint4& a, const uint4& b) {
    const u32x4_t av = __builtin_bit_cast(u32x4_t, a), bv = __builtin_bit_cast(u32x4_t, b);
    if constexpr (PREC == PREC_F16) {
        if constexpr (AG) asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+a"(c) : "v"(av), "v"(bv));
        else asm volatile("v_mfma_f32_32x32x16_f16 %0, %1, %2, %0" : "+v"(c) : "v"(av), "v"(bv));
    } else {
        if constexpr (AG) asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(av), "v"(bv));
        else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(av), "v"(bv));
    }
}

template <int PREC, bool OUT_F32, bool GELU>
__global__ __attribute__((amdgpu_flat_work_group_size(W4THREADS, W4THREADS), amdgpu_waves_per_eu(1, 1))) void gemm_et_w4_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, void* __restrict__ Cv,
    const float* __restrict__ bias, int M, int N, int K, int accumulate) {
    constexpr int NI = 5, NJ = 4;
    constexpr int XBN = 320;
    constexpr int XROWS = QBM + XBN;
    constexpr int XSTAGE_ELEMS = XROWS * XBK;
    constexpr uint32_t XSB = XSTAGE_ELEMS * 2;             // 72 KiB per stage
    constexpr int NP = 18, NP3 = 10;                       // pieces per wave and stage; [0, NP3) in step 3, the rest in step 0
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * XSTAGE_ELEMS];   // 144 KiB, ONE object

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;   // wave tile rows wm*128.., cols wn*160..

    constexpr int GROUP = 8;
    const int tiles_n = N / XBN, tiles_m = M / QBM, ntiles = tiles_n * tiles_m;
    const int per_group = GROUP * tiles_n;
#define W4_TILE(L_, m_, n_)                                                                      \
    do {                                                                                         \
        const int bid_ = xcd_remap((L_), ntiles);                                                \
        const int group_ = bid_ / per_group, first_m_ = group_ * GROUP;                           \
        const int gsz_ = (tiles_m - first_m_) < GROUP ? (tiles_m - first_m_) : GROUP;            \
        const int in_g_ = bid_ - group_ * per_group;                                             \
        (m_) = (first_m_ + in_g_ % gsz_) * QBM;                                                  \
        (n_) = (in_g_ / gsz_) * XBN;                                                             \
    } while (0)

    // DMA map: piece q of this wave covers stage rows 32 q + 8 wave .. + 7 (q < 8: A rows, else B rows 32 (q - 8) + ..); lane
    // l -> k-half l>>5, row (l>>2)&7, physical chunk l&3 (same image and swizzle as the eight-wave kernels: 32 q = 0 mod 16)
    const int prow = 8 * wave + ((lane >> 2) & 7);
    const uint32_t voff = ((uint32_t)prow * (uint32_t)K + (uint32_t)(lane >> 5) * 32u + (uint32_t)qswz(prow, lane & 3) * 8u) * 2u;
    const size_t rs32 = (size_t)32 * K;
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds + (uint32_t)wave * 1024u);
#define W4_PIECE(pa_, pb_, wr_, q_)                                                                        \
    glds16_m(voff, ((q_) < 8 ? (pa_) + (size_t)(q_) * rs32 : (pb_) + (size_t)((q_) - 8) * rs32), lds0 + (wr_) + (q_) * 4096u)

    const int nst = K / XBK;
    const int l31 = lane & 31, hh = lane >> 5;
    uint32_t offA[NJ], offB[NI];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { const int r = wm * 128 + j * 32 + l31; offA[j] = ((r >> 3) * 512 + (r & 7) * 32 + qswz(r, hh) * 8) * 2; }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int r = QBM + wn * 160 + i * 32 + l31;
        offB[i] = ((r >> 3) * 512 + (r & 7) * 32 + qswz(r, hh) * 8) * 2;
    }
    const unsigned char* ldsb = reinterpret_cast<const unsigned char*>(lds);

#define W4_RDB(fb_, rd_, s_, i_) fb_[i_] = *reinterpret_cast<const uint4*>(ldsb + (rd_) + ((s_) >> 1) * 512 + (offB[i_] ^ (((s_) & 1) * 32u)))
#define W4_RDA(fa_, rd_, s_, j_) fa_[j_] = *reinterpret_cast<const uint4*>(ldsb + (rd_) + ((s_) >> 1) * 512 + (offA[j_] ^ (((s_) & 1) * 32u)))
    // slot k (0..19) of a k-step: MFMA on accumulator tile (i = k % 5, j = k / 5) of the set (ca_, cb_); slots 0-8: one read of
    // the NEXT step's set; slots 10-19: DMA piece Q0_ + (k - 10) while < Q1_ (D_: 0 none, 1 always, 2 when dma_ is set)
#define W4_SLOT(k_, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                      \
        mfma32_asm<PREC, ((k_) % 5) < 4>(acc[(k_) % 5][(k_) / 5], cb_[(k_) % 5], ca_[(k_) / 5]);           \
        if constexpr ((k_) < 5) { W4_RDB(nb_, nrd_, ns_, ((k_) < 5 ? (k_) : 0)); }                         \
        else if constexpr ((k_) < 9) { W4_RDA(na_, nrd_, ns_, ((k_) >= 5 && (k_) < 9 ? (k_) - 5 : 0)); }   \
        if constexpr ((D_) != 0 && (k_) >= 10 && (Q0_) + (k_) - 10 < (Q1_)) {                              \
            if ((D_) == 1 || (dma_)) W4_PIECE(pa_, pb_, wr_, ((k_) >= 10 && (Q0_) + (k_) - 10 < NP ? (Q0_) + (k_) - 10 : 0)); \
        }                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);
#define W4_STEP(ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                          \
        W4_SLOT(0, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                       \
        W4_SLOT(1, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                       \
        W4_SLOT(2, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                       \
        W4_SLOT(3, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                       \
        W4_SLOT(4, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                       \
        W4_SLOT(5, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                       \
        W4_SLOT(6, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                       \
        W4_SLOT(7, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                       \
        W4_SLOT(8, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                       \
        W4_SLOT(9, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                       \
        W4_SLOT(10, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                      \
        W4_SLOT(11, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                      \
        W4_SLOT(12, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                      \
        W4_SLOT(13, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                      \
        W4_SLOT(14, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                      \
        W4_SLOT(15, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                      \
        W4_SLOT(16, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                      \
        W4_SLOT(17, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                      \
        W4_SLOT(18, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)                      \
        W4_SLOT(19, ca_, cb_, na_, nb_, nrd_, ns_, D_, dma_, Q0_, Q1_, pa_, pb_, wr_)
#define W4_STAGE(D0_, d0_, a0_, b0_, D3_, d3_, a3_, b3_)                                                   \
        {                                                                                                  \
            const uint32_t ot = XSB - rd;                                                                  \
            W4_STEP(fa0, fb0, fa1, fb1, rd, 1, D0_, d0_, NP3, NP, a0_, b0_, ot)                            \
            W4_STEP(fa1, fb1, fa0, fb0, rd, 2, 0, false, 0, 0, a0_, b0_, ot)                               \
            W4_STEP(fa0, fb0, fa1, fb1, rd, 3, 0, false, 0, 0, a0_, b0_, ot)                               \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                    \
            __builtin_amdgcn_s_barrier();                                                                  \
            __builtin_amdgcn_sched_barrier(0);                                                             \
            W4_STEP(fa1, fb1, fa0, fb0, ot, 0, D3_, d3_, 0, NP3, a3_, b3_, rd)                             \
            rd = ot;                                                                                       \
        }
#define W4_ISSUE_RANGE(pa_, pb_, wr_, LO, HI)                                                              \
    do {                                                                                                   \
        _Pragma("unroll") for (int q_ = 0; q_ < NP; ++q_)                                                  \
            if (q_ >= (LO) && q_ < (HI)) {                                                                 \
                glds16_m(voff, (q_ < 8 ? (pa_) + (size_t)q_ * rs32 : (pb_) + (size_t)(q_ - 8) * rs32), lds0 + (wr_) + q_ * 4096u); \
            }                                                                                              \
    } while (0)

    int L = blockIdx.x, m0, n0;
    W4_TILE(L, m0, n0);
    const uint16_t* sA = A + (size_t)m0 * K;
    const uint16_t* sB = B + (size_t)n0 * K;
    W4_ISSUE_RANGE(sA, sB, 0u, 0, NP);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    f32x16_t acc[NI][NJ];
    for (;;) {
        const int Ln = L + (int)gridDim.x;
        const bool more = Ln < ntiles;
        int m1 = m0, n1 = n0;
        if (more) W4_TILE(Ln, m1, n1);
        const uint16_t* nA = A + (size_t)m1 * K;
        const uint16_t* nB = B + (size_t)n1 * K;
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        {
            const uint16_t* a1 = sA + XBK;
            const uint16_t* b1 = sB + XBK;
            W4_ISSUE_RANGE(a1, b1, XSB, 0, NP3);           // early pieces of stage 1 -> buffer 1
        }
        uint4 fa0[NJ], fb0[NI], fa1[NJ], fb1[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) W4_RDB(fb0, 0u, 0, i);
#pragma unroll
        for (int j = 0; j < NJ; ++j) W4_RDA(fa0, 0u, 0, j);
        // accumulator writes (VALU / v_accvgpr_write) before the first MFMA: same tie
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (j == NJ - 1)
                asm volatile("s_nop 7" : "+a"(acc[0][j]), "+a"(acc[1][j]), "+a"(acc[2][j]), "+a"(acc[3][j]), "+v"(acc[4][j]));
            else
                asm volatile("" : "+a"(acc[0][j]), "+a"(acc[1][j]), "+a"(acc[2][j]), "+a"(acc[3][j]), "+v"(acc[4][j]));
        }
        __builtin_amdgcn_sched_barrier(0);
        uint32_t rd = 0;
        const uint16_t* pa = sA + XBK;
        const uint16_t* pb = sB + XBK;
        for (int t = 0; t + 2 < nst; ++t) {
            W4_STAGE(1, true, pa, pb, 1, true, pa + XBK, pb + XBK)
            pa += XBK;
            pb += XBK;
        }
        W4_STAGE(1, true, pa, pb, 2, more, nA, nB)         // t = nst-2
        W4_STAGE(2, more, nA, nB, 0, false, nA, nB)        // t = nst-1
        // The last MFMA results must not be read for 18 wait states, and hipcc neither knows that the asm statements above are
        // MFMAs nor keeps register-only code behind a bare asm: the padding is tied to every accumulator tile by data dependence.
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (j == 0)
                asm volatile("s_nop 15\n\ts_nop 15" : "+a"(acc[0][j]), "+a"(acc[1][j]), "+a"(acc[2][j]), "+a"(acc[3][j]), "+v"(acc[4][j]));
            else
                asm volatile("" : "+a"(acc[0][j]), "+a"(acc[1][j]), "+a"(acc[2][j]), "+a"(acc[3][j]), "+v"(acc[4][j]));
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            unsigned char* scr = reinterpret_cast<unsigned char*>(lds) + XSB + wave * (XSB / 4);
            epilogue_m32<PREC, OUT_F32, GELU, false, NJ>(acc, scr, Cv, bias, N, m0 + wm * 128, n0 + wn * 160, wn, accumulate, lane);
        }
        if (!more) break;
        __builtin_amdgcn_s_barrier();
        L = Ln; m0 = m1; n0 = n1; sA = nA; sB = nB;
    }
#undef W4_TILE
#undef W4_PIECE
#undef W4_RDA
#undef W4_RDB
#undef W4_SLOT
#undef W4_STEP
#undef W4_STAGE
#undef W4_ISSUE_RANGE
}

template <int PREC>
hipError_t launch_gemm_w4(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, bool out_f32, bool gelu,
                          bool accumulate, bool persistent, hipStream_t s) {
    const int ntiles = (M / QBM) * (N / WBN);
    const int n_cu = cu_count();
    dim3 grid(persistent && ntiles > n_cu ? n_cu : ntiles), block(W4THREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    const int acc = accumulate ? 1 : 0;
    if (out_f32) {
        if (gelu) gemm_et_w4_kernel<PREC, true, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc);
        else gemm_et_w4_kernel<PREC, true, false><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc);
    } else {
        if (gelu) gemm_et_w4_kernel<PREC, false, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc);
        else gemm_et_w4_kernel<PREC, false, false><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc);
    }
    return hipGetLastError();
}

// producer of the folded LayerNorm: C = A B^T + bias + C (fp32), Xh = ET(C), stats[m][N / 160] = (mean, M2) per 160 columns
template <int PREC>
hipError_t launch_gemm_m32_stats(const void* A, const void* B, float* C, const float* bias, void* Xh, float* stats,
                                 int M, int N, int K, int spread, hipStream_t s) {
    const int ntiles = (M / QBM) * (N / WBN);
    const int n_cu = cu_count_now();
    dim3 grid(ntiles > n_cu ? n_cu : ntiles), block(QTHREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    if (spread) gemm_et_m32_kernel<PREC, true, false, 1, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, 1, reinterpret_cast<uint16_t*>(Xh), reinterpret_cast<float2*>(stats));
    else gemm_et_m32_kernel<PREC, true, false, 0, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, 1, reinterpret_cast<uint16_t*>(Xh), reinterpret_cast<float2*>(stats));
    return hipGetLastError();
}

// LayerNorm folded into the neighbouring GEMMs (ViT-H: the residual stream has N = 1280 = LN_NS x 160 columns).
constexpr int LN_NS = 8;                       // 1280 / 160: ViT-H only

}  // namespace

namespace gemm_fam {

hipError_t m32(int prec, int spread, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, bool out_f32, bool gelu,
               bool accumulate, bool persistent, hipStream_t s) {
    return with_prec(prec, [&](auto P) -> hipError_t {
        if (spread) return launch_gemm_m32<P.value, 1>(A, B, C, bias, M, N, K, out_f32, gelu, accumulate, persistent, s);
        return launch_gemm_m32<P.value, 0>(A, B, C, bias, M, N, K, out_f32, gelu, accumulate, persistent, s);
    });
}

hipError_t w4(int prec, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, bool out_f32, bool gelu,
              bool accumulate, bool persistent, hipStream_t s) {
    return with_prec(prec, [&](auto P) { return launch_gemm_w4<P.value>(A, B, C, bias, M, N, K, out_f32, gelu, accumulate, persistent, s); });
}

}  // namespace gemm_fam

hipError_t launch_gemm_et_stats(int prec, const void* A, const void* B, float* C, const float* bias, void* Xh, float* stats,
                                int M, int N, int K, hipStream_t s) {
    if (!m32_ok(M, N, K, false) || N != 160 * LN_NS || !Xh || !stats) return hipErrorInvalidValue;
    static const int spread = [] { const char* v = getenv("SAMRS_GEMM_M32"); return v ? ((atoi(v) & 8) ? 1 : 0) : 1; }();
    return with_prec(prec, [&](auto P) { return launch_gemm_m32_stats<P.value>(A, B, C, bias, Xh, stats, M, N, K, spread, s); });
}
hipError_t launch_gemm_et_fold(int prec, const void* Xh, const void* Wf, void* C, const float* bias_f, const float* cvec,
                               const float* rowstat, int M, int N, int K, bool gelu, hipStream_t s) {
    if (M % QBM || N % WBN || K != 160 * LN_NS || !bias_f || !cvec || !rowstat) return hipErrorInvalidValue;
    return gemm_fam::x64p_fold(prec, Xh, Wf, C, bias_f, cvec, rowstat, M, N, K, gelu, s);
}
#endif  // SAMRS_EXPERIMENTS
