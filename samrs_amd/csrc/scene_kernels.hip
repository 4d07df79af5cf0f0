// scene_kernels.hip -- compositing the masks of several windows of one large scene into the scene's own frame (gfx950).
//
// A scene larger than the encoder's input is decoded window by window (samrs_amd/scene.py); every box is decoded in exactly one
// window.  The reference's rule for the class map -- boxes are painted in annotation order, a later box wins
// (Generate Dataset/main_sam_hbox_semantic.py:162,195-199) -- has to hold ACROSS windows, whatever the order the windows are
// decoded in.  So the scene keeps an int32 map `order` [H][W] (-1 = unclaimed) of the highest annotation rank set at each pixel:
//   scene_claim_kernel    one predict call's masks [n][h][w], all decoded in the window (x0, y0, w, h): a thread owns 16 adjacent
//                         pixels of one window row, walks the n masks once (16-byte loads where w % 16 == 0), counts each mask's
//                         set bytes (area) and keeps the largest rank set at each of its pixels, then does ONE read-max-write of
//                         its 16 map entries.  A pixel has one owner per call and the calls on a map are stream-ordered: no
//                         atomics on the map, and max is commutative, so the map does not depend on the order of the calls.
//   scene_resolve_kernel  seg[p] = order[p] < 0 ? 255 : label of rank order[p].
// Integer work bounded by bytes: n h w mask bytes read once, 4 h w map bytes read and written once per call.
// Areas: per-wave shuffle sum -> LDS counter per mask -> one device-scope atomicAdd per block and mask (integer: exact and
// order-independent), as paint_area_kernel does.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int SC_CHUNK = 64;          // masks per LDS counter chunk
constexpr int SC_PIX = 16;            // pixels of a window row per thread
constexpr int SC_UNROLL = 4;          // masks whose loads a thread issues together

__device__ __forceinline__ uint32_t sc_nonzero_bytes(uint32_t w) {      // 0x80 in every byte of w that is not 0
    return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;
}
__device__ __forceinline__ unsigned int sc_wave_sum(unsigned int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// VEC: w % 16 == 0 and 16-byte aligned masks (launcher).  Thread t of the grid: window row t / G, pixels 16 (t % G) .. + 15,
// G = ceil(w / 16).  Every thread of a block takes part in the reductions, also the ones past the window.
template <bool VEC>
__global__ __launch_bounds__(256) void scene_claim_kernel(const uint8_t* __restrict__ masks, const int32_t* __restrict__ ranks, int n,
                                                          int h, int w, int x0, int y0, int W, int32_t* __restrict__ order,
                                                          unsigned long long* __restrict__ areas) {
    __shared__ unsigned int cnt_s[SC_CHUNK];
    const int G = (w + SC_PIX - 1) / SC_PIX;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int row = (int)(t / G), xs = (int)(t % G) * SC_PIX;
    const bool in = row < h;
    const int npx = in ? (w - xs < SC_PIX ? w - xs : SC_PIX) : 0;
    const size_t hw = (size_t)h * w, p0 = (size_t)(in ? row : 0) * w + xs;
    int best[SC_PIX];
#pragma unroll
    for (int k = 0; k < SC_PIX; ++k) best[k] = -1;
    for (int jlo = 0; jlo < n; jlo += SC_CHUNK) {
        const int jhi = jlo + SC_CHUNK < n ? jlo + SC_CHUNK : n;
        if (areas) {
            if (threadIdx.x < SC_CHUNK) cnt_s[threadIdx.x] = 0u;
            __syncthreads();
        }
        for (int j0 = jlo; j0 < jhi; j0 += SC_UNROLL) {
            // the loads of SC_UNROLL masks are issued before any of them is used: one thread has that many 16-byte loads in flight.
            // Measured on 32 masks of 1024^2: 27.9 us against 28.6 us with one load at a time (6.7 us from bytes alone) -- the loads'
            // latency is not what bounds this kernel at one block per CU; profiles/scene_bench.txt
            uint32_t wd[SC_UNROLL][4];
            int r[SC_UNROLL];
#pragma unroll
            for (int u = 0; u < SC_UNROLL; ++u) {
                wd[u][0] = wd[u][1] = wd[u][2] = wd[u][3] = 0u;
                r[u] = -1;
                if (in && j0 + u < jhi) {
                    r[u] = ranks[j0 + u];
                    if (VEC) {
                        const uint4 m = *reinterpret_cast<const uint4*>(masks + (size_t)(j0 + u) * hw + p0);
                        wd[u][0] = m.x; wd[u][1] = m.y; wd[u][2] = m.z; wd[u][3] = m.w;
                    } else {
                        const uint8_t* src = masks + (size_t)(j0 + u) * hw + p0;
#pragma unroll
                        for (int k = 0; k < SC_PIX; ++k)
                            if (k < npx) wd[u][k >> 2] |= (uint32_t)src[k] << (8 * (k & 3));
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < SC_UNROLL; ++u) {
                if (j0 + u >= jhi) break;                                 // uniform over the block
                unsigned int cnt = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t tb = sc_nonzero_bytes(wd[u][q]);
                    cnt += __popc(tb);
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int cand = (tb >> (8 * c + 7)) & 1u ? r[u] : -1;
                        best[4 * q + c] = best[4 * q + c] > cand ? best[4 * q + c] : cand;
                    }
                }
                if (areas) {
                    const unsigned int c = sc_wave_sum(cnt);          // <= 1024
                    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&cnt_s[j0 + u - jlo], c);
                }
            }
        }
        if (areas) {
            __syncthreads();
            if (threadIdx.x < jhi - jlo && cnt_s[threadIdx.x]) atomicAdd(&areas[jlo + threadIdx.x], (unsigned long long)cnt_s[threadIdx.x]);
            __syncthreads();
        }
    }
    if (!in) return;
    int any = -1;
#pragma unroll
    for (int k = 0; k < SC_PIX; ++k) any = any > best[k] ? any : best[k];
    if (any < 0) return;                                               // nothing set here: the map keeps what it has
    int32_t* dst = order + (size_t)(y0 + row) * W + x0 + xs;
    if (npx == SC_PIX && (((uintptr_t)dst) & 15) == 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int4 o = reinterpret_cast<int4*>(dst)[q];
            o.x = o.x > best[4 * q] ? o.x : best[4 * q];
            o.y = o.y > best[4 * q + 1] ? o.y : best[4 * q + 1];
            o.z = o.z > best[4 * q + 2] ? o.z : best[4 * q + 2];
            o.w = o.w > best[4 * q + 3] ? o.w : best[4 * q + 3];
            reinterpret_cast<int4*>(dst)[q] = o;
        }
    } else {
#pragma unroll
        for (int k = 0; k < SC_PIX; ++k)
            if (k < npx && best[k] > dst[k]) dst[k] = best[k];
    }
}

// statistic.py:18-21 (area > 0 only), as samrs_paint accumulates them
__global__ void scene_class_stats_kernel(const unsigned long long* __restrict__ areas, const int32_t* __restrict__ labels, int n,
                                         unsigned long long* __restrict__ cpix, unsigned long long* __restrict__ cins, int n_classes) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int j = 0; j < n; ++j) {
        const int l = labels[j];
        if (areas[j] > 0 && l >= 0 && l < n_classes) {
            if (cpix) cpix[l] += areas[j];
            if (cins) cins[l] += 1ull;
        }
    }
}

__device__ __forceinline__ uint32_t sc_label(int o, const int32_t* __restrict__ labels_by_rank, int n_ranks) {
    return (o < 0 || o >= n_ranks) ? 255u : (uint32_t)(uint8_t)labels_by_rank[o];
}
// a thread resolves 4 adjacent pixels (16-byte map load, 4-byte store); the last hw % 4 pixels one by one
__global__ __launch_bounds__(256) void scene_resolve_kernel(const int32_t* __restrict__ order, const int32_t* __restrict__ labels_by_rank,
                                                            int n_ranks, long hw, uint8_t* __restrict__ seg, int vec) {
    const long n4 = vec ? hw / 4 : 0;
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const int4 o = reinterpret_cast<const int4*>(order)[i];
        reinterpret_cast<uint32_t*>(seg)[i] = sc_label(o.x, labels_by_rank, n_ranks) | (sc_label(o.y, labels_by_rank, n_ranks) << 8) |
                                              (sc_label(o.z, labels_by_rank, n_ranks) << 16) | (sc_label(o.w, labels_by_rank, n_ranks) << 24);
    }
    for (long p = 4 * n4 + (long)blockIdx.x * 256 + threadIdx.x; p < hw; p += stride)
        seg[p] = (uint8_t)sc_label(order[p], labels_by_rank, n_ranks);
}

}  // namespace

hipError_t launch_scene_claim(const uint8_t* masks, const int32_t* ranks, const int32_t* labels, int n, int h, int w, int x0, int y0,
                              int H, int W, int32_t* order, unsigned long long* areas, unsigned long long* class_pixels,
                              unsigned long long* class_instances, int n_classes, hipStream_t s) {
    if (n < 0 || h < 1 || w < 1 || x0 < 0 || y0 < 0 || x0 > W - w || y0 > H - h) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    if (areas) HIP_CHECK_RET(hipMemsetAsync(areas, 0, sizeof(unsigned long long) * n, s));
    const long threads = (long)h * ((w + SC_PIX - 1) / SC_PIX);
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    if (w % 16 == 0 && (((uintptr_t)masks) & 15) == 0)
        scene_claim_kernel<true><<<blocks, 256, 0, s>>>(masks, ranks, n, h, w, x0, y0, W, order, areas);
    else
        scene_claim_kernel<false><<<blocks, 256, 0, s>>>(masks, ranks, n, h, w, x0, y0, W, order, areas);
    if (areas && (class_pixels || class_instances))
        scene_class_stats_kernel<<<1, 64, 0, s>>>(areas, labels, n, class_pixels, class_instances, n_classes);
    return hipGetLastError();
}

hipError_t launch_scene_resolve(const int32_t* order, const int32_t* labels_by_rank, int n_ranks, int H, int W, uint8_t* seg,
                                hipStream_t s) {
    if (n_ranks < 0 || H < 1 || W < 1) return hipErrorInvalidValue;
    const long hw = (long)H * W;
    const int vec = ((((uintptr_t)order) & 15) == 0 && (((uintptr_t)seg) & 3) == 0) ? 1 : 0;
    long blocks = ((vec ? hw / 4 : hw) + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    scene_resolve_kernel<<<(unsigned)blocks, 256, 0, s>>>(order, labels_by_rank, n_ranks, hw, seg, vec);
    return hipGetLastError();
}
