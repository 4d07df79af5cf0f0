// gemm_device.h -- what more than one of the gemm*.hip sources uses (internal to them; the launchers between them: gemm_families.h).
// Everything here is __device__ __forceinline__, inline or a constant, and sits in the anonymous namespace like the kernels
// themselves: each translation unit gets its own copy.  A helper that one file alone uses lives in that file.
#pragma once

#include <cstdlib>

#include <type_traits>

#include "common.h"
#include "gemm_select.h"
#include "kernels.h"

using namespace gemm_sel;

namespace gemm_fam {
// CUs of the current device, asked per call / once per process.  Defined in gemm.hip: the function-local static is one per process,
// not one per file.
int cu_count_now();
int cu_count();
}  // namespace gemm_fam

namespace {

using gemm_fam::cu_count;
using gemm_fam::cu_count_now;

// f(std::integral_constant<int, PREC_*>) for the operand type named at run time
template <class F>
hipError_t with_prec(int prec, F&& f) {
    if (prec == PREC_BF16) return f(std::integral_constant<int, PREC_BF16>{});
    if (prec == PREC_F16) return f(std::integral_constant<int, PREC_F16>{});
    return hipErrorInvalidValue;
}
template <int V>
using Int = std::integral_constant<int, V>;

// threads and ring depth of the eight-wave 256-row kernels (gemm.hip; gemm_et_m32_kernel in gemm_experiments.hip)
constexpr int QSTAGES = 4, QTHREADS = 512;     // WBN = 320: the NI = 5 flavour, 256x320 tile (wave tile 128x80), 4 x 36 KiB ring

// swizzle of an LDS image with 64-byte rows: 16-byte chunk index XORed with g(row >> 2), g = [0,2,3,1] (why: gemm_et_big_kernel,
// gemm.hip; the pair-stage, four-wave, dual and MX kernels keep the same geometry inside a k-half)
__device__ __forceinline__ int qswz(int r, int c) { return c ^ ((0x78 >> (2 * ((r >> 2) & 3))) & 3); }

// the four-wave kernels (gemm_et_w4x_kernel in gemm.hip; gemm_et_w4_kernel in gemm_experiments.hip): one wave per SIMD
constexpr int W4THREADS = 256;
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));

// LDS-DMA issued from inline asm so that hipcc's s_waitcnt insertion does not know about it (it
// would otherwise put vmcnt(0) in front of every ds_read).  M0 = LDS byte address of the wave's
// 1 KiB destination; M0 is compiler-reserved, so it is saved / restored inside the statement, and
// the SALU-write -> LDS-DMA hazard gets its s_nop (cdna_hip_programming.md 5.7).  The caller
// counts vmcnt by hand.
template <int OFF>
__device__ __forceinline__ void glds16_asm(const uint16_t* gsrc, uint32_t wave_lds_base) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_add_u32 m0, %2, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(wave_lds_base), "n"(OFF)
        : "memory", "scc");
}

// LDS-DMA, scalar-base form: source = sbase (SGPR pair, wave-uniform) + voff (per-lane byte offset, one VGPR),
// destination = LDS byte address m0v (wave-uniform) + 16 * lane.  Issued from inline asm for the same reason as
// glds16_asm (hipcc must not see it in its waitcnt bookkeeping); the caller counts vmcnt by hand.
__device__ __forceinline__ void glds16_s(uint32_t voff, const void* sbase, uint32_t m0v) {
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(sbase), "s"(m0v)
        : "memory");
}

// LDS-DMA piece with M0 declared as clobbered instead of saved / restored (two SALU instructions less per piece)
__device__ __forceinline__ void glds16_m(uint32_t voff, const void* sbase, uint32_t m0v) {
    asm volatile(
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %0, %1"
        :
        : "v"(voff), "s"(sbase), "s"(m0v)
        : "memory", "m0");
}

__device__ __forceinline__ void wave_lds_sync_g() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------------------------
// Coalesced epilogue.  In the MFMA accumulator layout a lane owns 4 consecutive columns of ONE row,
// so a direct store instruction scatters 16 rows x 32-byte pieces: measured (ablation)
// that costs a third of the whole GEMM.  Instead each wave bounces its 64-column sub-tile through
// its private slice of the (now idle) LDS ring and writes / read-modify-writes FULL 128- or 256-byte
// row segments with 16 bytes per lane.  bias + GELU are applied before the bounce (per-lane column
// known), the 2-D addend and the residual accumulate after it (coalesced loads).
//   acc[i][j]: n-tile i (16 cols), m-tile j (16 rows); NJ m-tiles per wave, JC of them per pass.
// ---------------------------------------------------------------------------------------------
// DRAIN (persistent kernels): the caller has LDS-DMA pieces of its NEXT tile in flight; they are retired (vmcnt(0)) right
// before this wave's first global store, i.e. after the bias loads, the VALU work and the first LDS bounce have covered
// their latency, and before any store joins the queue -- so the stores themselves are never waited for.
template <int PREC, bool OUT_F32, int GELU /* 0 none, 1 fp32-epsilon erf, 2 the cheaper erf (ET output) */, int NJ, int JC, int NI = 4, bool GLN = false,
          bool DRAIN = false, bool STREAM = false /* ET output: non-temporal stores (common.h store16_stream) */>
__device__ __forceinline__ void epilogue_coalesced(f32x4_t (&acc)[NI][NJ], unsigned char* scr /* wave-private */,
                                                   void* __restrict__ Cv, const float* __restrict__ bias,
                                                   const float* __restrict__ add2d, int add2d_period, int N,
                                                   int m_base /* first row of the wave tile */,
                                                   int n_base /* first column of the wave tile */, int accumulate,
                                                   int lane, const float* __restrict__ pre2d = nullptr /* ET output: 2-D addend
                                                   applied before the bounce, loaded element by element (keeps registers low) */) {
    const int fr = lane & 15, fq = lane >> 4;
    // padded row stride: the smallest >= the 16*NI-column row with (words % 32) == 4, which spreads the 16
    // rows of an accumulator column block over all banks (NI = 4: 272 / 144 bytes)
    constexpr int ROWW = 16 * NI * (OUT_F32 ? 4 : 2) / 4;
    constexpr int RS = (((ROWW - 4 + 31) / 32) * 32 + 4) * 4;
    constexpr int TS = 16 * RS;                                     // one m-tile
    constexpr int CPR = 16 * NI * (OUT_F32 ? 4 : 2) / 16;           // 16-byte chunks per row segment
    constexpr int NCH = 16 * CPR, NPASS = (NCH + 63) / 64;
    float4 bv[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
        bv[i] = bias ? *reinterpret_cast<const float4*>(bias + n_base + i * 16 + 4 * fq) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j0 = 0; j0 < NJ; j0 += JC) {
        // fp32 output: the residual (old C) and the 2-D addend of this pass do not depend on the accumulators --
        // issue their loads FIRST, so that they are in flight during the LDS bounce instead of after it
        float4 res[OUT_F32 ? JC : 1][OUT_F32 ? NPASS : 1];
        if (OUT_F32) {
#pragma unroll
            for (int jj = 0; jj < JC; ++jj)
#pragma unroll
                for (int h = 0; h < NPASS; ++h) {
                    const int idx = lane + 64 * h;
                    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (NCH % 64 == 0 || idx < NCH) {
                        const int m = m_base + (j0 + jj) * 16 + idx / CPR, n = n_base + (idx % CPR) * 4;
                        if (accumulate) r = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(Cv) + (size_t)m * N + n);
                        if (add2d && !GLN) {      // GLN: `add2d` carries gamma | beta, not a 2-D addend
                            const float4 e = *reinterpret_cast<const float4*>(add2d + (size_t)(m % add2d_period) * N + n);
                            r.x += e.x; r.y += e.y; r.z += e.z; r.w += e.w;
                        }
                    }
                    res[jj][h] = r;
                }
        }
        if (j0) wave_lds_sync_g();
#pragma unroll
        for (int jj = 0; jj < JC; ++jj) {
            const int j = j0 + jj;
            // GLN: LayerNorm2d over the wave's 64 columns (= one channel group of the transposed-conv output,
            // mask_decoder.py:55-56, eps 1e-6) before the GELU.  A row's 64 values sit in the 4 lane quarters x
            // 16 registers; two-pass statistics like the stand-alone kernel.  `add2d` carries gamma[64] | beta[64].
            float gmean = 0.f, grstd = 1.f;
            if (GLN) {
                float s1 = 0.f;
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    s1 += ((acc[i][j][0] + bv[i].x) + (acc[i][j][1] + bv[i].y)) + ((acc[i][j][2] + bv[i].z) + (acc[i][j][3] + bv[i].w));
                s1 += __shfl_xor(s1, 16, 64);
                s1 += __shfl_xor(s1, 32, 64);
                gmean = s1 * (1.0f / 64.0f);
                float s2 = 0.f;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const float a0 = acc[i][j][0] + bv[i].x - gmean, a1 = acc[i][j][1] + bv[i].y - gmean;
                    const float a2 = acc[i][j][2] + bv[i].z - gmean, a3 = acc[i][j][3] + bv[i].w - gmean;
                    s2 += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
                }
                s2 += __shfl_xor(s2, 16, 64);
                s2 += __shfl_xor(s2, 32, 64);
                grstd = 1.0f / sqrtf(s2 * (1.0f / 64.0f) + 1e-6f);
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                float v0 = acc[i][j][0] + bv[i].x, v1 = acc[i][j][1] + bv[i].y;
                float v2 = acc[i][j][2] + bv[i].z, v3 = acc[i][j][3] + bv[i].w;
                if (pre2d) {
                    const float4 e = *reinterpret_cast<const float4*>(pre2d + (size_t)((m_base + j * 16 + fr) % add2d_period) * N +
                                                                      n_base + i * 16 + 4 * fq);
                    v0 += e.x; v1 += e.y; v2 += e.z; v3 += e.w;
                }
                if (GLN) {
                    const float4 gm = *reinterpret_cast<const float4*>(add2d + i * 16 + 4 * fq);
                    const float4 bt = *reinterpret_cast<const float4*>(add2d + 64 + i * 16 + 4 * fq);
                    v0 = (v0 - gmean) * grstd * gm.x + bt.x; v1 = (v1 - gmean) * grstd * gm.y + bt.y;
                    v2 = (v2 - gmean) * grstd * gm.z + bt.z; v3 = (v3 - gmean) * grstd * gm.w + bt.w;
                }
                if constexpr (GELU == 2 && !OUT_F32) { const float2_t g01 = gelu_erf2_et(float2_t{v0, v1}), g23 = gelu_erf2_et(float2_t{v2, v3}); v0 = g01.x; v1 = g01.y; v2 = g23.x; v3 = g23.y; }
                else if constexpr (GELU != 0) { const float2_t g01 = gelu_erf2(float2_t{v0, v1}), g23 = gelu_erf2(float2_t{v2, v3}); v0 = g01.x; v1 = g01.y; v2 = g23.x; v3 = g23.y; }
                unsigned char* p = scr + jj * TS + fr * RS;
                if (OUT_F32) {
                    *reinterpret_cast<float4*>(p + (i * 16 + 4 * fq) * 4) = make_float4(v0, v1, v2, v3);
                } else {
                    uint2 o;
                    o.x = pack2<PREC>(v0, v1);
                    o.y = pack2<PREC>(v2, v3);
                    *reinterpret_cast<uint2*>(p + (i * 16 + 4 * fq) * 2) = o;
                }
            }
        }
        wave_lds_sync_g();
        if (DRAIN && j0 == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
        for (int jj = 0; jj < JC; ++jj) {
            const int j = j0 + jj;
            if (OUT_F32) {
                // 16 rows x (64 NI) B in 16-byte chunks, consecutive lanes on consecutive chunks of a row
#pragma unroll
                for (int h = 0; h < NPASS; ++h) {
                    const int idx = lane + 64 * h;
                    if (NCH % 64 != 0 && idx >= NCH) break;
                    const int row = idx / CPR, ch = idx % CPR;
                    float4 v = *reinterpret_cast<const float4*>(scr + jj * TS + row * RS + ch * 16);
                    const int m = m_base + j * 16 + row, n = n_base + ch * 4;
                    const float4 o = res[OUT_F32 ? jj : 0][OUT_F32 ? h : 0];
                    v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w;
                    float* C = reinterpret_cast<float*>(Cv) + (size_t)m * N + n;
                    *reinterpret_cast<float4*>(C) = v;
                }
            } else {
                // 16 rows x (32 NI) B
#pragma unroll
                for (int h = 0; h < NPASS; ++h) {
                    const int idx = lane + 64 * h;
                    if (NCH % 64 != 0 && idx >= NCH) break;
                    const int row = idx / CPR, ch = idx % CPR;
                    const uint4 v = *reinterpret_cast<const uint4*>(scr + jj * TS + row * RS + ch * 16);
                    uint16_t* C = reinterpret_cast<uint16_t*>(Cv) + (size_t)(m_base + j * 16 + row) * N + n_base + ch * 8;
                    store16_stream<STREAM>(C, v);
                }
            }
        }
    }
}

}  // namespace
