// overlap_kernels.hip -- one instance per pixel: where several masks of one predict call are set at a pixel, the pixel is given to
// exactly one of them and cleared in the others, in place (gfx950).  samrs_resolve_overlaps (samrs_hip.h) states the rule; in short,
// walking the masks j = 0 .. n-1 with a holder b per pixel, mask j (its byte set at p) takes the pixel iff there is no holder, or
// P[j] > P[b], or P[j] == P[b] and not v_j(p) < v_b(p): P an int64 key per mask, v the postprocessed logit (postprocess_value.h --
// the statements postprocess_kernel expands, so v is the value the mask byte was thresholded from).  Ties go to the later mask.
//   overlap_area_kernel     the set bytes of every mask on entry (before_out, and the key of the smallest-first rule).
//   overlap_resolve_kernel  the thread geometry of scene_claim_kernel: a thread owns 16 adjacent pixels of one row as four 4-pixel
//                           groups (X0 % 4 == 0, what the macro needs); 16-byte mask loads where w % 16 == 0.  A pixel has exactly
//                           one owning thread: no atomics on masks or map, no dependence on launch order.
//     pass A   every thread walks the n masks once and keeps, per pixel, "some mask set", "two or more set" (byte flags) and the
//              last mask set.  A block none of whose pixels is contested writes owner_out and is done: the common case, bound by
//              reading n h w mask bytes once.
//     pass B1  only threads with a contested pixel, only their contested groups, only the masks pass A saw set at one of the thread's
//              pixels (a 64-bit word, bit j % 64): those masks again (4-byte words), v for the ones that compete in the group (256 KiB
//              of logits per mask, L2-resident), the sequential rule, the winner per pixel.
//     pass B2  the losers' bytes cleared, again over the set bits only; only words that changed are stored.  removed: per-wave shuffle sum -> LDS counter per mask
//              in chunks of 64 masks -> one device-scope atomicAdd per block and mask, as scene_claim_kernel counts its areas.
// Integer atomics only, and every float comparison is made by one thread from values it computed itself: bitwise reproducible.
#include "common.h"
#include "kernels.h"
#include "postprocess_value.h"

namespace {

constexpr int OV_CHUNK = 64;          // masks per LDS counter chunk
constexpr int OV_PIX = 16;            // pixels of a row per thread
constexpr int OV_UNROLL = 4;          // masks whose loads a thread issues together (pass A)

__device__ __forceinline__ uint32_t ov_nonzero_bytes(uint32_t w) {      // 0x80 in every byte of w that is not 0
    return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;
}
__device__ __forceinline__ uint32_t ov_byte_mask(uint32_t flags) {      // 0xFF in every byte whose 0x80 flag is set
    return (flags >> 7) * 0xFFu;
}
__device__ __forceinline__ unsigned int ov_wave_sum(unsigned int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ unsigned long long ov_wave_or(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
    return v;
}
static_assert(OV_CHUNK == 64, "bit k of a thread's `bits` stands for the masks j with j % 64 == k: one counter chunk per 64-bit word");

// the 16 pixels of a thread as four words (byte c of word q = pixel 4 q + c; pixels past npx read as 0)
template <bool VEC>
__device__ __forceinline__ void ov_load16(const uint8_t* __restrict__ src, int npx, uint32_t (&wd)[4]) {
    if (VEC) {
        const uint4 m = *reinterpret_cast<const uint4*>(src);
        wd[0] = m.x; wd[1] = m.y; wd[2] = m.z; wd[3] = m.w;
    } else {
        wd[0] = wd[1] = wd[2] = wd[3] = 0u;
#pragma unroll
        for (int k = 0; k < OV_PIX; ++k)
            if (k < npx) wd[k >> 2] |= (uint32_t)src[k] << (8 * (k & 3));
    }
}
// one group of 4 pixels (src points at the group; nq = pixels of it inside the row)
template <bool VEC>
__device__ __forceinline__ uint32_t ov_load4(const uint8_t* src, int nq) {
    if (VEC) return *reinterpret_cast<const uint32_t*>(src);
    uint32_t wd = 0u;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (c < nq) wd |= (uint32_t)src[c] << (8 * c);
    return wd;
}

// Thread t of the grid: row t / G, pixels 16 (t % G) .. + 15, G = ceil(W / 16).  Every thread of a block takes part in the
// reductions, also the ones past the image.
template <bool VEC>
__global__ __launch_bounds__(256) void overlap_area_kernel(const uint8_t* __restrict__ masks, int n, int H, int W,
                                                           unsigned long long* __restrict__ areas) {
    __shared__ unsigned int cnt_s[OV_CHUNK];
    const int G = (W + OV_PIX - 1) / OV_PIX;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int row = (int)(t / G), xs = (int)(t % G) * OV_PIX;
    const bool in = row < H;
    const int npx = in ? (W - xs < OV_PIX ? W - xs : OV_PIX) : 0;
    const size_t hw = (size_t)H * W, p0 = (size_t)(in ? row : 0) * W + xs;
    for (int jlo = 0; jlo < n; jlo += OV_CHUNK) {
        const int jhi = jlo + OV_CHUNK < n ? jlo + OV_CHUNK : n;
        if (threadIdx.x < OV_CHUNK) cnt_s[threadIdx.x] = 0u;
        __syncthreads();
        for (int j0 = jlo; j0 < jhi; j0 += OV_UNROLL) {
            uint32_t wd[OV_UNROLL][4];
#pragma unroll
            for (int u = 0; u < OV_UNROLL; ++u) {
                wd[u][0] = wd[u][1] = wd[u][2] = wd[u][3] = 0u;
                if (in && j0 + u < jhi) ov_load16<VEC>(masks + (size_t)(j0 + u) * hw + p0, npx, wd[u]);
            }
#pragma unroll
            for (int u = 0; u < OV_UNROLL; ++u) {
                if (j0 + u >= jhi) break;                                 // uniform over the block
                unsigned int cnt = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) cnt += __popc(ov_nonzero_bytes(wd[u][q]));
                const unsigned int c = ov_wave_sum(cnt);              // <= 1024
                if ((threadIdx.x & 63) == 0 && c) atomicAdd(&cnt_s[j0 + u - jlo], c);
            }
        }
        __syncthreads();
        if (threadIdx.x < jhi - jlo && cnt_s[threadIdx.x]) atomicAdd(&areas[jlo + threadIdx.x], (unsigned long long)cnt_s[threadIdx.x]);
        __syncthreads();
    }
}

// prim: the int64 key per mask, or null (every key equal); prim_neg: the key is -prim[j] (prim = the entry areas: smallest first).
// low_all: fp32 [n][LS][LS] or null (no logit term: equal).  removed: zeroed by the launcher, or null.
template <bool VEC>
__global__ __launch_bounds__(256) void overlap_resolve_kernel(uint8_t* __restrict__ masks, int n, int H, int W,
                                                              const long long* __restrict__ prim, int prim_neg,
                                                              const float* __restrict__ low_all, int LS, int in_h, int in_w, int img_size,
                                                              int32_t* __restrict__ owner_out, unsigned long long* __restrict__ removed) {
    __shared__ unsigned int cnt_s[OV_CHUNK];
    const int G = (W + OV_PIX - 1) / OV_PIX;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int row = (int)(t / G), xs = (int)(t % G) * OV_PIX;
    const bool in = row < H;
    const int npx = in ? (W - xs < OV_PIX ? W - xs : OV_PIX) : 0;
    const size_t hw = (size_t)H * W, p0 = (size_t)(in ? row : 0) * W + xs;

    // ---- pass A: per pixel "set somewhere", "set twice or more", the last mask set; per thread `bits`: bit j % 64 = mask j is set
    // at one of its pixels -- the only masks passes B1 / B2 have to look at again (a box-prompted mask covers few threads)
    uint32_t seen[4] = {0u, 0u, 0u, 0u}, multi[4] = {0u, 0u, 0u, 0u};
    unsigned long long bits = 0ull;
    int own[OV_PIX];
#pragma unroll
    for (int k = 0; k < OV_PIX; ++k) own[k] = -1;
    if (in) {
        for (int j0 = 0; j0 < n; j0 += OV_UNROLL) {
            uint32_t wd[OV_UNROLL][4];
#pragma unroll
            for (int u = 0; u < OV_UNROLL; ++u) {
                wd[u][0] = wd[u][1] = wd[u][2] = wd[u][3] = 0u;
                if (j0 + u < n) ov_load16<VEC>(masks + (size_t)(j0 + u) * hw + p0, npx, wd[u]);
            }
#pragma unroll
            for (int u = 0; u < OV_UNROLL; ++u) {
                if (wd[u][0] | wd[u][1] | wd[u][2] | wd[u][3]) bits |= 1ull << ((j0 + u) & 63);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t tb = ov_nonzero_bytes(wd[u][q]);
                    multi[q] |= seen[q] & tb;
                    seen[q] |= tb;
#pragma unroll
                    for (int c = 0; c < 4; ++c) own[4 * q + c] = (tb >> (8 * c + 7)) & 1u ? j0 + u : own[4 * q + c];
                }
            }
        }
    }
    const bool contested = (multi[0] | multi[1] | multi[2] | multi[3]) != 0u;

    // ---- pass B1: the rule on the contested groups of the threads that have one
    if (contested) {
#pragma unroll 1
        for (int q = 0; q < 4; ++q) {
            const uint32_t mq = q == 0 ? multi[0] : q == 1 ? multi[1] : q == 2 ? multi[2] : multi[3];
            if (!mq) continue;
            const int nq = npx - 4 * q < 4 ? npx - 4 * q : 4;             // >= 1: the group holds a set pixel
            int hold[4] = {-1, -1, -1, -1};
            long long pb[4] = {0, 0, 0, 0};
            float vb[4] = {0.f, 0.f, 0.f, 0.f};
            // ascending j over the masks whose bit is set: 64 masks per word of `bits`, its set bits from the lowest
            for (int base = 0; base < n; base += 64) {
                for (unsigned long long left = bits; left; left &= left - 1) {
                    const int j = base + __ffsll(left) - 1;
                    if (j >= n) break;
                    const uint32_t cand = ov_nonzero_bytes(ov_load4<VEC>(masks + (size_t)j * hw + p0 + 4 * q, nq)) & mq;
                    if (!cand) continue;
                    long long pj = 0;
                    if (prim) pj = prim_neg ? -prim[j] : prim[j];
                    float vj[4] = {0.f, 0.f, 0.f, 0.f};
                    if (low_all) {
                        const float* low = low_all + (size_t)j * LS * LS;
                        // Y and X0 do not change over j, and the compiler hoists every coordinate, weight and offset of the macro's
                        // three routes out of this loop: > 256 VGPRs for the whole kernel, pass A included (one wave per SIMD).  Made
                        // opaque they are recomputed per competing mask, here only: 122 VGPRs, no scratch.
                        int Y = row, X0 = xs + 4 * q;
                        asm volatile("" : "+v"(Y), "+v"(X0));
                        SAMRS_POSTPROCESS_VALUES();
#pragma unroll
                        for (int e = 0; e < 4; ++e) vj[e] = v[e];
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (!((cand >> (8 * e + 7)) & 1u)) continue;
                        const bool take = hold[e] < 0 || pj > pb[e] || (pj == pb[e] && !(vj[e] < vb[e]));
                        if (take) {
                            hold[e] = j;
                            pb[e] = pj;
                            vb[e] = vj[e];
                        }
                    }
                }
            }
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                if (qq != q) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if ((mq >> (8 * e + 7)) & 1u) own[4 * qq + e] = hold[e];
            }
        }
    }

    // ---- the owner map: the winner where a mask is set, -1 elsewhere
    if (owner_out && in) {
        int32_t* dst = owner_out + p0;
        if (npx == OV_PIX && (((uintptr_t)dst) & 15) == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) reinterpret_cast<int4*>(dst)[q] = make_int4(own[4 * q], own[4 * q + 1], own[4 * q + 2], own[4 * q + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < OV_PIX; ++k)
                if (k < npx) dst[k] = own[k];
        }
    }
    if (!__syncthreads_or(contested ? 1 : 0)) return;                 // nothing to clear in this block: the common case

    // ---- pass B2: clear the losers; removed[j] counted per wave -> LDS -> one atomic per block and mask
    const unsigned long long wave_bits = ov_wave_or(contested ? bits : 0ull);        // wave-uniform: the masks this wave may clear
    for (int jlo = 0; jlo < n; jlo += OV_CHUNK) {
        const int jhi = jlo + OV_CHUNK < n ? jlo + OV_CHUNK : n;
        if (removed) {
            if (threadIdx.x < OV_CHUNK) cnt_s[threadIdx.x] = 0u;
            __syncthreads();
        }
        for (unsigned long long left = wave_bits; left; left &= left - 1) {      // jlo % 64 == 0: bit k is mask jlo + k
            const int k = __ffsll(left) - 1, j = jlo + k;
            if (j >= jhi) break;
            unsigned int cnt = 0;
            if (contested && ((bits >> k) & 1ull)) {
                uint8_t* mj = masks + (size_t)j * hw + p0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    if (!multi[q]) continue;
                    const int nq = npx - 4 * q < 4 ? npx - 4 * q : 4;
                    const uint32_t wd = ov_load4<VEC>(mj + 4 * q, nq);
                    uint32_t lose = ov_nonzero_bytes(wd) & multi[q];
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (own[4 * q + c] == j) lose &= ~(0x80u << (8 * c));
                    if (!lose) continue;
                    cnt += __popc(lose);
                    if (VEC) {
                        *reinterpret_cast<uint32_t*>(mj + 4 * q) = wd & ~ov_byte_mask(lose);
                    } else {
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if ((lose >> (8 * c + 7)) & 1u) mj[4 * q + c] = 0;      // a set byte: inside the row
                    }
                }
            }
            if (removed) {
                const unsigned int c = ov_wave_sum(cnt);              // <= 1024
                if ((threadIdx.x & 63) == 0 && c) atomicAdd(&cnt_s[j - jlo], c);
            }
        }
        if (removed) {
            __syncthreads();
            if (threadIdx.x < jhi - jlo && cnt_s[threadIdx.x]) atomicAdd(&removed[jlo + threadIdx.x], (unsigned long long)cnt_s[threadIdx.x]);
            __syncthreads();
        }
    }
}

}  // namespace

hipError_t launch_mask_areas(const uint8_t* masks, int n, int h, int w, unsigned long long* areas, hipStream_t s) {
    if (!masks || !areas || n < 1 || h < 1 || w < 1 || (long)h * w >= (1l << 31)) return hipErrorInvalidValue;
    HIP_CHECK_RET(hipMemsetAsync(areas, 0, sizeof(unsigned long long) * (size_t)n, s));
    const long threads = (long)h * ((w + OV_PIX - 1) / OV_PIX);
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    if (w % 16 == 0 && (((uintptr_t)masks) & 15) == 0) overlap_area_kernel<true><<<blocks, 256, 0, s>>>(masks, n, h, w, areas);
    else overlap_area_kernel<false><<<blocks, 256, 0, s>>>(masks, n, h, w, areas);
    return hipGetLastError();
}

hipError_t launch_resolve_overlaps(uint8_t* masks, int n, int h, int w, const long long* prim, int prim_neg, const float* low, int in_h,
                                   int in_w, int img_size, int32_t* owner_out, unsigned long long* removed, hipStream_t s) {
    if (!masks || n < 1 || h < 1 || w < 1 || (long)h * w >= (1l << 31)) return hipErrorInvalidValue;
    if (low && (in_h < 1 || in_w < 1 || img_size < 4)) return hipErrorInvalidValue;
    if (removed) HIP_CHECK_RET(hipMemsetAsync(removed, 0, sizeof(unsigned long long) * (size_t)n, s));
    const long threads = (long)h * ((w + OV_PIX - 1) / OV_PIX);
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    const int LS = img_size / 4;
    if (w % 16 == 0 && (((uintptr_t)masks) & 15) == 0)
        overlap_resolve_kernel<true><<<blocks, 256, 0, s>>>(masks, n, h, w, prim, prim_neg, low, LS, in_h, in_w, img_size, owner_out, removed);
    else
        overlap_resolve_kernel<false><<<blocks, 256, 0, s>>>(masks, n, h, w, prim, prim_neg, low, LS, in_h, in_w, img_size, owner_out, removed);
    return hipGetLastError();
}
