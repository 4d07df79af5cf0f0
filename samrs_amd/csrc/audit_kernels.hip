// audit_kernels.hip -- checkpoint audit (engine options "range_profile" / "audit_passes"; include/samrs_hip.h samrs_audit_*).
// Two diagnostic passes over MFMA-operand tensors (uint16 bit patterns, f16 or bf16), written like the range scan in
// encoder_kernels.hip: 16-byte loads, grid-stride, no per-element global traffic.  Every sum that crosses a block is an INTEGER atomic
// or a plain store followed by an ordered sum: two runs over the same tensor give the same bits.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int PROFILE_BINS = 40;          // floor(log2 |x|) = -24 ... 15  ->  bin 0 ... 39

// ---- range_profile_kernel -------------------------------------------------------------------------------------------------
// One profile row of AUDIT_PROFILE_WORDS int64 per tensor (layout: samrs_hip.h samrs_audit_read_profile).  The four class counters and
// the running maximum live in registers; the 40 exponent bins live in LDS with ONE COUNTER PER LANE ([wave][bin][lane], 40 KB): a lane
// only ever touches its own words, so a tensor whose elements all share one exponent costs what any other tensor costs -- no two lanes
// of a wave meet on an address, and bank = lane for every bin.  At the end each wave folds ten bins over the four waves' copies
// (conflict-free reads + a shuffle tree), and the block issues one 64-bit integer atomic per NON-EMPTY counter.
template <int PREC>
__device__ __forceinline__ void profile_element(uint32_t m /* bits & 0x7fff */, uint32_t* __restrict__ my_bins /* &bins[wave][0][lane] */,
                                                unsigned& zeros, unsigned& subs, unsigned& at_max, unsigned& infnan, uint32_t& top) {
    constexpr int MANT = PREC == PREC_F16 ? 10 : 7;
    constexpr uint32_t EXP_ALL = PREC == PREC_F16 ? 31u : 255u, MAX_FINITE = PREC == PREC_F16 ? 0x7bffu : 0x7f7fu;
    constexpr int BIAS = PREC == PREC_F16 ? 15 : 127;
    if (m == 0) { ++zeros; return; }
    const uint32_t ex = m >> MANT;
    if (ex == EXP_ALL) { ++infnan; return; }
    int lg;                                // floor(log2 |x|)
    if (ex == 0) {                         // subnormal: |x| = m * 2^(1 - BIAS - MANT)
        ++subs;
        lg = (31 - __clz((int)m)) + 1 - BIAS - MANT;
    } else
        lg = (int)ex - BIAS;
    const int b = lg < -24 ? 0 : lg > 15 ? PROFILE_BINS - 1 : lg + 24;
    my_bins[b * 64] += 1;
    at_max += m == MAX_FINITE;
    top = m > top ? m : top;
}

template <int PREC>
__global__ __launch_bounds__(256) void range_profile_kernel(const uint4* __restrict__ x, long n16, unsigned long long* __restrict__ row,
                                                            int row16 /* live 16-byte units per row */, int ld16 /* row stride in 16-byte units */) {
    __shared__ uint32_t bins[4][PROFILE_BINS][64];
    __shared__ unsigned cls[4][4];
    __shared__ uint32_t tops[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int b = 0; b < PROFILE_BINS; ++b) bins[wave][b][lane] = 0;
    uint32_t* my_bins = &bins[wave][0][lane];
    unsigned zeros = 0, subs = 0, at_max = 0, infnan = 0, seen = 0;
    uint32_t top = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256) {
        // rows with a stride: only the first row16 units of every ld16 are operand values (range_scan_kernel's addressing)
        const uint4 v = x[row16 == ld16 ? i : (i / row16) * ld16 + i % row16];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            profile_element<PREC>(w[k] & 0x7fffu, my_bins, zeros, subs, at_max, infnan, top);
            profile_element<PREC>((w[k] >> 16) & 0x7fffu, my_bins, zeros, subs, at_max, infnan, top);
        }
        seen += 8;
    }
    // the class counters: per wave by shuffle, per block through LDS (a thread sees at most 2^31 / 256 elements per launch: no overflow)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        zeros += __shfl_xor(zeros, off, 64); subs += __shfl_xor(subs, off, 64);
        at_max += __shfl_xor(at_max, off, 64); infnan += __shfl_xor(infnan, off, 64);
        const uint32_t o = __shfl_xor(top, off, 64);
        top = o > top ? o : top;
    }
    // `seen` is summed as 64-bit: a block may scan more than 2^32 elements in principle
    unsigned long long seen64 = seen;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) seen64 += __shfl_xor(seen64, off, 64);
    __shared__ unsigned long long seen_w[4];
    if (lane == 0) {
        cls[wave][0] = zeros; cls[wave][1] = subs; cls[wave][2] = at_max; cls[wave][3] = infnan;
        tops[wave] = top; seen_w[wave] = seen64;
    }
    __syncthreads();
    // bins: wave w folds bins 10 w ... 10 w + 9 over the four waves' copies
    for (int j = 0; j < PROFILE_BINS / 4; ++j) {
        const int b = wave * (PROFILE_BINS / 4) + j;
        unsigned long long t = (unsigned long long)bins[0][b][lane] + bins[1][b][lane] + bins[2][b][lane] + bins[3][b][lane];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
        if (lane == 0 && t) atomicAdd(&row[8 + b], t);
    }
    if (threadIdx.x < 4) {
        const unsigned long long t = (unsigned long long)cls[0][threadIdx.x] + cls[1][threadIdx.x] + cls[2][threadIdx.x] + cls[3][threadIdx.x];
        if (t) atomicAdd(&row[1 + threadIdx.x], t);
    } else if (threadIdx.x == 4) {
        const unsigned long long t = seen_w[0] + seen_w[1] + seen_w[2] + seen_w[3];
        if (t) atomicAdd(&row[0], t);
    } else if (threadIdx.x == 5) {
        uint32_t t = tops[0];
        for (int w = 1; w < 4; ++w) t = tops[w] > t ? tops[w] : t;
        if (t) atomicMax(&row[5], (unsigned long long)t);
    }
}

// ---- column statistics of a GEMM A operand [M][K] ---------------------------------------------------------------------------
// Stage one: a block of one wave owns a slab of at most AUDIT_ROWS_PER_PARTIAL rows x 512 columns, a lane 8 neighbouring columns (one
// 16-byte load per row; a wave reads 1 KB of a row at a time).  x^2 is accumulated per column in fp32 IN ROW ORDER (f16 and bf16 squares
// are exact in fp32; the only rounding is this chain: at most (rows - 1) half-ulps relative, every addend being non-negative) and stored
// with plain stores to partials[slab][K].  The largest magnitude pattern goes to maxbits[c] with an integer atomicMax, skipped when the
// word already holds as much (monotonic, so a stale read only costs an atomic).
// Stage two: one thread per column adds the slab partials in slab order into the fp64 total sumsq[c].
template <int PREC>
__global__ __launch_bounds__(64) void column_stats_kernel(const uint16_t* __restrict__ x, int M, int K, int ld, float* __restrict__ partials,
                                                          uint32_t* __restrict__ maxbits) {
    const int c0 = (blockIdx.x * 64 + threadIdx.x) * 8;
    if (c0 >= K) return;
    const int slab = blockIdx.y, r0 = slab * AUDIT_ROWS_PER_PARTIAL;
    const int r1 = r0 + AUDIT_ROWS_PER_PARTIAL < M ? r0 + AUDIT_ROWS_PER_PARTIAL : M;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t top[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint16_t* p = x + (size_t)r0 * ld + c0;
    auto take = [&](const uint4& v) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const uint32_t bits = h ? w[k] >> 16 : w[k] & 0xffffu;
                const float f = ET<PREC>::to_float((uint16_t)bits);
                acc[2 * k + h] += f * f;
                const uint32_t m = bits & 0x7fffu;
                top[2 * k + h] = m > top[2 * k + h] ? m : top[2 * k + h];
            }
        }
    };
    int r = r0;
    for (; r + 8 <= r1; r += 8, p += (size_t)8 * ld) {        // eight loads in flight, consumed in row order
        uint4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = *reinterpret_cast<const uint4*>(p + (size_t)j * ld);
#pragma unroll
        for (int j = 0; j < 8; ++j) take(v[j]);
    }
    for (; r < r1; ++r, p += ld) take(*reinterpret_cast<const uint4*>(p));
    float* out = partials + (size_t)slab * K + c0;
    *reinterpret_cast<float4*>(out) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4*>(out + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (top[j] > maxbits[c0 + j]) atomicMax(&maxbits[c0 + j], top[j]);
}

__global__ __launch_bounds__(256) void column_stats_reduce_kernel(const float* __restrict__ partials, int n_slabs, int K, double* __restrict__ sumsq) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= K) return;
    double t = sumsq[c];
    for (int s = 0; s < n_slabs; ++s) t += (double)partials[(size_t)s * K + c];
    sumsq[c] = t;
}

}  // namespace

hipError_t launch_range_profile(int prec, const void* x, long n, int cols, int ld, long long* row48, hipStream_t s) {
    // n elements in all as rows of `cols` live elements stored with a stride of `ld` (cols <= 0: one dense run)
    if (cols <= 0) { cols = 8; ld = 8; }
    if (n < 0 || n % 8 || !x || !row48 || cols % 8 || ld % 8 || ld < cols || n % cols || ((uintptr_t)x & 15)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const long n16 = n / 8;
    long blocks = (n16 + 256 * 8 - 1) / (256 * 8);
    if (blocks > 1024) blocks = 1024;       // three 40 KB blocks fit a CU's LDS: a little over one resident round on 256 CUs
    unsigned long long* row = reinterpret_cast<unsigned long long*>(row48);
    if (prec == PREC_BF16) range_profile_kernel<PREC_BF16><<<(int)blocks, 256, 0, s>>>(reinterpret_cast<const uint4*>(x), n16, row, cols / 8, ld / 8);
    else range_profile_kernel<PREC_F16><<<(int)blocks, 256, 0, s>>>(reinterpret_cast<const uint4*>(x), n16, row, cols / 8, ld / 8);
    return hipGetLastError();
}

size_t column_stats_partial_floats(int M, int K) {
    return (size_t)((M + AUDIT_ROWS_PER_PARTIAL - 1) / AUDIT_ROWS_PER_PARTIAL) * K;
}

hipError_t launch_column_stats(int prec, const void* x, int M, int K, int ld, float* partials, double* sumsq, uint32_t* maxbits, hipStream_t s) {
    if (!x || !partials || !sumsq || !maxbits || M < 1 || K < 8 || K % 8 || ld % 8 || ld < K || ((uintptr_t)x & 15) || ((uintptr_t)partials & 15))
        return hipErrorInvalidValue;
    const int n_slabs = (M + AUDIT_ROWS_PER_PARTIAL - 1) / AUDIT_ROWS_PER_PARTIAL;
    if (n_slabs > 65535) return hipErrorInvalidValue;
    const dim3 grid((K / 8 + 63) / 64, n_slabs);
    if (prec == PREC_BF16) column_stats_kernel<PREC_BF16><<<grid, 64, 0, s>>>((const uint16_t*)x, M, K, ld, partials, maxbits);
    else column_stats_kernel<PREC_F16><<<grid, 64, 0, s>>>((const uint16_t*)x, M, K, ld, partials, maxbits);
    hipError_t r = hipGetLastError();
    if (r != hipSuccess) return r;
    column_stats_reduce_kernel<<<(K + 255) / 256, 256, 0, s>>>(partials, n_slabs, K, sumsq);
    return hipGetLastError();
}
