// gemm_families.h -- the launchers launch_gemm_et's switch (gemm.hip) calls in the other gemm sources.  A kernel template cannot be
// instantiated across translation units, so each takes the operand type (and GLDS / GROUP_M / STAG / SPREAD where the kernel has them
// as template parameters) at run time and picks the instantiation in its own file; a value it has no instantiation for is
// hipErrorInvalidValue.  Arguments are what launch_gemm_et was given (kernels.h).
#pragma once

#include <hip/hip_runtime.h>

namespace gemm_fam {

// gemm_ring.hip: 128 x 128 (glds: LDS-DMA staging; group_m = 1 | 8: grouped tile order) and 256 x 128
hipError_t base(int prec, bool glds, int group_m, const void* A, const void* B, void* C, const float* bias, const float* add2d, int period,
                int M, int N, int K, bool out_f32, bool gelu, bool accumulate, hipStream_t s);
hipError_t stag(int prec, const void* A, const void* B, void* C, const float* bias, const float* add2d, int period,
                int M, int N, int K, bool out_f32, bool gelu, bool accumulate, hipStream_t s);

// gemm_dual.hip: 2 blocks / CU; stag = false: one barrier per K step
hipError_t dual(int prec, bool stag, const void* A, const void* B, void* C, const float* bias, const float* add2d, int period,
                int M, int N, int K, bool out_f32, bool gelu, bool accumulate, hipStream_t s);

// gemm_decoder.hip: K = 256 streaming
hipError_t k256(int prec, const void* A, const void* B, void* C, const float* bias, const float* add2d, int period,
                int M, int N, hipStream_t s);

#ifdef SAMRS_EXPERIMENTS
// gemm_experiments.hip: the 32x32x16 kernels
hipError_t m32(int prec, int spread, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, bool out_f32, bool gelu,
               bool accumulate, bool persistent, hipStream_t s);
hipError_t w4(int prec, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, bool out_f32, bool gelu,
              bool accumulate, bool persistent, hipStream_t s);
// gemm.hip, for launch_gemm_et_fold (gemm_experiments.hip): the consumer of the folded LayerNorm on the persistent pair-stage kernel
hipError_t x64p_fold(int prec, const void* A, const void* B, void* C, const float* bias, const float* cvec, const float* rowstat,
                     int M, int N, int K, bool gelu, hipStream_t s);
#endif

}  // namespace gemm_fam
