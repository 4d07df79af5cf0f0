// quality_kernels.hip -- per-mask quality signals counted on the device, and the gate that uses them (gfx950).
//
// samrs_score_masks: the reference's stability score (utils/amg.py:156-176) is the IoU of the mask thresholded at +offset and at
// -offset, taken at the full output resolution.  Materialising fp32 logits for that costs 4 MiB per 1024^2 mask; here the counts
// come straight from the 256^2 logits (256 KiB per mask, L2-resident) and 32 bytes per mask are written:
//   score_masks_kernel   grid (chunks, n).  A thread takes 4 horizontally adjacent output pixels per step of a grid-stride loop and
//                        computes their values with SAMRS_POSTPROCESS_VALUES (postprocess_value.h) -- the statements
//                        postprocess_kernel expands, so `v > 0` here and the mask byte there agree on every pixel
//                        (tests/test_quality_gpu.py asks for exact equality on every route).  The four predicates (v > +offset,
//                        v > 0, v > -offset, v > 0 inside the box) are counted per wave with __ballot (64-bit) + __popcll into
//                        wave-uniform counters, summed over the block's 4 waves through LDS, and each block issues ONE 64-bit
//                        integer atomicAdd per counter: <= SCORE_BLOCKS * 4 atomics per mask.  Integer only: exact, and the same
//                        whatever the order of the blocks.
// What bounds it has NOT been measured.  The expectation, from counting instructions: about 16 loads (L2 / L1 hits: neighbouring
// pixels share their logits) and ~60 fp32 / integer VALU operations per pixel on the two-stage route, 8 loads per 4 pixels on the
// identity route -- VALU / interpolation bound, not bandwidth bound.
//
// samrs_filter_masks: filter_masks_kernel, grid (chunks, n): every block evaluates mask j's rule from its 32 bytes of counts (fp64
// comparisons of integers against fp32 thresholds), block 0 writes keep[j], and the blocks of a dropped mask zero it with 16-byte
// stores (VEC) or byte stores.  A kept mask is neither read nor written.
#include "common.h"
#include "kernels.h"
#include "postprocess_value.h"

namespace {

constexpr int SCORE_BLOCKS = 64;        // blocks per mask at most: 256 atomics per mask however large it is
constexpr int FILTER_BLOCKS = 64;

__global__ __launch_bounds__(256) void score_masks_kernel(const float* __restrict__ low_all, int LS, int in_h, int in_w, int H, int W,
                                                          int img_size, float offset, const float* __restrict__ boxes,
                                                          unsigned long long* __restrict__ counts) {
    __shared__ unsigned int part[4][4];                   // [wave][counter]
    const int W4 = (W + 3) / 4;
    const long total = (long)W4 * H;
    const int mi = blockIdx.y;
    const float* low = low_all + (size_t)mi * LS * LS;
    // no box: an inverted one, which holds no pixel
    const float bx0 = boxes ? boxes[4 * mi + 0] : 1.f, by0 = boxes ? boxes[4 * mi + 1] : 1.f;
    const float bx1 = boxes ? boxes[4 * mi + 2] : 0.f, by1 = boxes ? boxes[4 * mi + 3] : 0.f;
    const float neg = -offset;
    unsigned int c_hi = 0, c_mid = 0, c_lo = 0, c_in = 0;                // wave-uniform; < 2^31 (H * W < 2^31)
    // every thread of the block makes the same number of steps: the ballots below are never under divergent control flow
    for (long t0 = (long)blockIdx.x * 256; t0 < total; t0 += (long)gridDim.x * 256) {
        const long t = t0 + threadIdx.x;
        const bool act = t < total;
        int Yt = 0, Xt = 0;
        float val[4] = {0.f, 0.f, 0.f, 0.f};
        if (act) {
            const int Y = (int)(t / W4), X0 = (int)(t % W4) * 4;
            SAMRS_POSTPROCESS_VALUES();
#pragma unroll
            for (int e = 0; e < 4; ++e) val[e] = v[e];
            Yt = Y;
            Xt = X0;
        }
        const float fy = (float)Yt;
        const bool row_in = by0 <= fy && fy <= by1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool ok = act && Xt + e < W;
            const float fx = (float)(Xt + e);
            const bool mid = ok && val[e] > 0.f;
            c_hi += (unsigned int)__popcll(__ballot(ok && val[e] > offset));
            c_mid += (unsigned int)__popcll(__ballot(mid));
            c_lo += (unsigned int)__popcll(__ballot(ok && val[e] > neg));
            c_in += (unsigned int)__popcll(__ballot(mid && row_in && bx0 <= fx && fx <= bx1));
        }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = c_hi;
        part[wave][1] = c_mid;
        part[wave][2] = c_lo;
        part[wave][3] = c_in;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long sum = (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] +
                                       part[3][threadIdx.x];
        if (sum) atomicAdd(&counts[(size_t)mi * 4 + threadIdx.x], sum);
    }
}

__device__ __forceinline__ bool keep_rule(const long long* __restrict__ c, const float* __restrict__ iou, int j, float min_stability,
                                          float min_pred_iou, float min_inside) {
    const long long n_hi = c[0], n_mid = c[1], n_lo = c[2], n_in = c[3];
    bool keep = true;
    if (min_stability > 0.f) keep = keep && n_lo > 0 && (double)n_hi >= (double)min_stability * (double)n_lo;
    if (min_pred_iou > 0.f) keep = keep && iou[j] > min_pred_iou;
    if (min_inside > 0.f) keep = keep && (n_mid == 0 || (double)n_in >= (double)min_inside * (double)n_mid);
    return keep;
}

// VEC: masks 16-byte aligned and hw % 16 == 0 (launcher): every mask starts on a 16-byte boundary
template <bool VEC>
__global__ __launch_bounds__(256) void filter_masks_kernel(uint8_t* __restrict__ masks, long hw, const long long* __restrict__ counts,
                                                           const float* __restrict__ iou, float min_stability, float min_pred_iou,
                                                           float min_inside, uint8_t* __restrict__ keep_out) {
    const int j = blockIdx.y;
    const bool keep = keep_rule(counts + (size_t)j * 4, iou, j, min_stability, min_pred_iou, min_inside);    // block-uniform
    if (blockIdx.x == 0 && threadIdx.x == 0) keep_out[j] = keep ? 1 : 0;
    if (keep) return;
    uint8_t* m = masks + (size_t)j * hw;
    const long stride = (long)gridDim.x * 256;
    if (VEC) {
        uint4* m4 = reinterpret_cast<uint4*>(m);
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < hw / 16; p += stride) m4[p] = z;
    } else {
        for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < hw; p += stride) m[p] = 0;
    }
}

}  // namespace

hipError_t launch_score_masks(const float* low, int n, int in_h, int in_w, int orig_h, int orig_w, int img_size, float offset,
                              const float* boxes, unsigned long long* counts, hipStream_t s) {
    if (!low || !counts || n < 1 || in_h < 1 || in_w < 1 || orig_h < 1 || orig_w < 1 || img_size < 4) return hipErrorInvalidValue;
    if ((long)orig_h * orig_w >= (1l << 31)) return hipErrorInvalidValue;
    HIP_CHECK_RET(hipMemsetAsync(counts, 0, sizeof(unsigned long long) * 4 * (size_t)n, s));
    const int LS = img_size / 4;
    const long work = (long)((orig_w + 3) / 4) * orig_h;
    const long blocks = (work + 255) / 256;
    const unsigned gx = (unsigned)(blocks < SCORE_BLOCKS ? blocks : SCORE_BLOCKS);
    for (int off = 0; off < n; off += 32768) {             // gridDim.y <= 65535
        const int m = n - off < 32768 ? n - off : 32768;
        dim3 g(gx, (unsigned)m), b(256);
        score_masks_kernel<<<g, b, 0, s>>>(low + (size_t)off * LS * LS, LS, in_h, in_w, orig_h, orig_w, img_size, offset,
                                           boxes ? boxes + (size_t)off * 4 : nullptr, counts + (size_t)off * 4);
    }
    return hipGetLastError();
}

hipError_t launch_filter_masks(uint8_t* masks, int n, long hw, const long long* counts, const float* iou, float min_stability,
                               float min_pred_iou, float min_inside, uint8_t* keep, hipStream_t s) {
    if (!masks || !counts || !keep || n < 1 || hw < 1 || (min_pred_iou > 0.f && !iou)) return hipErrorInvalidValue;
    const bool vec = hw % 16 == 0 && ((uintptr_t)masks & 15) == 0;
    const long work = vec ? hw / 16 : hw;
    const long blocks = (work + 255) / 256;
    const unsigned gx = (unsigned)(blocks < FILTER_BLOCKS ? blocks : FILTER_BLOCKS);
    for (int off = 0; off < n; off += 32768) {
        const int m = n - off < 32768 ? n - off : 32768;
        dim3 g(gx, (unsigned)m), b(256);
        uint8_t* mp = masks + (size_t)off * hw;
        const long long* cp = counts + (size_t)off * 4;
        const float* ip = iou ? iou + off : nullptr;
        if (vec) filter_masks_kernel<true><<<g, b, 0, s>>>(mp, hw, cp, ip, min_stability, min_pred_iou, min_inside, keep + off);
        else filter_masks_kernel<false><<<g, b, 0, s>>>(mp, hw, cp, ip, min_stability, min_pred_iou, min_inside, keep + off);
    }
    return hipGetLastError();
}
