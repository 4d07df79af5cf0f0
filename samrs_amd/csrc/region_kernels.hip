// region_kernels.hip -- small-region removal on full-resolution binary masks on the device (gfx950).
//
// Restates `remove_small_regions` of Generate Dataset/segment_anything/utils/amg.py:267-291 (cv2.connectedComponentsWithStats,
// 8-connectivity) for a batch of masks that never leave HBM:
//   holes   : every unset pixel in an 8-connected component of the COMPLEMENT with fewer than T pixels becomes set;
//   islands : every set pixel in an 8-connected component with fewer than T pixels is cleared; if EVERY component is small, exactly
//             one survives, the largest (amg.py:287-289).
// Tie rule (ours): of several largest components the one whose first pixel in row-major order comes first survives.  The
// reference takes np.argmax over cv2's label numbers, and cv2 does not promise their order, so it has no rule to restate.
//
// Connected-component labelling is a block-based union-find; a component's label is its smallest row-major pixel index, whatever
// order the unions arrive in, so every output is bitwise reproducible.  Per pass over a chunk of masks, separate launches on the
// caller's stream (every cross-workgroup dependence is a kernel boundary; no grid barrier, no spin-wait):
//   1. region_local_kernel   one workgroup per 32 x 128 tile: 16-byte mask reads, union-find in LDS (atomicMin on 16 KB of int32),
//                            label = smallest pixel index of the TILE-local component.  Uniform tiles take no iteration.
//   2. region_merge_kernel   thread = pixel on the first row / first column of a tile: unions with the three neighbours across the
//                            border (diagonals across tile corners included), device-scope atomicMin on the label array.
//   3. region_area_kernel    every label that a pixel holds is re-pointed at its root (afterwards root(p) = L[L[p]], two loads:
//                            only the tile-local roots are rewritten, not the 4 bytes of every pixel), and area[root] += pixels,
//                            one integer atomicAdd per wave and root after a match of the lanes' runs.
//   4. region_reduce_kernel  (islands) per mask: "is any component >= T", and the largest component as one 64-bit atomicMax on
//                            (area << 32) | (0xffffffff - root) -- which is the tie rule above.
//   5. region_apply_kernel   rewrites the mask in place as 0 / 1 (16-byte loads and stores), counts pixels set and pixels changed.
// Every union-find loop is bounded by the chain it walks: labels only ever decrease.  Integer arithmetic only: bit-exact with
// tests/region_ref.py (tests/test_clean_masks_gpu.py).  h * w < 2^30 (int32 pixel indices); any h, w >= 1.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int RG_TH = 32, RG_TW = 128;            // tile: 4096 pixels, 256 threads x 16 pixels of one row
constexpr int RG_SEGS = RG_TW / 16;               // threads per tile row

struct RegionCtr {                                 // per mask of a chunk, zeroed before every pass
    unsigned long long best;                       // (area << 32) | (0xffffffff - root) of the largest component
    unsigned long long set;                        // pixels set after the cleanup
    unsigned long long changed;                    // pixels whose value changed
    unsigned int any_big;                          // a component with area >= T exists
    unsigned int pad;
};

__device__ __forceinline__ uint32_t rg_nz_bytes(uint32_t w) {      // 0x80 in every byte of w that is not 0
    return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;
}
// bit i = byte i of the 16 bytes is not 0
__device__ __forceinline__ uint32_t rg_nz_bits16(const uint32_t q[4]) {
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t t = rg_nz_bytes(q[k]) >> 7;                 // 0x01 per non-zero byte
        bits |= ((t & 1u) | ((t >> 7) & 2u) | ((t >> 14) & 4u) | ((t >> 21) & 8u)) << (4 * k);
    }
    return bits;
}

// the 16 pixels (y, x .. x + 15) of one mask -> bit i = pixel x + i is set; *valid = bit i: x + i < w.  VEC: w % 16 == 0 and a
// 16-byte aligned base, so the segment is whole and aligned.
template <bool VEC>
__device__ __forceinline__ uint32_t rg_load_bits(const uint8_t* __restrict__ row, int x, int w, uint32_t* valid, uint32_t raw[4]) {
    raw[0] = raw[1] = raw[2] = raw[3] = 0u;
    if (VEC) {
        const uint4 q = *reinterpret_cast<const uint4*>(row + x);
        raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
        *valid = 0xFFFFu;
    } else {
        const int nv = w - x < 16 ? w - x : 16;
        for (int i = 0; i < nv; ++i) raw[i >> 2] |= (uint32_t)row[x + i] << (8 * (i & 3));
        *valid = (1u << nv) - 1u;
    }
    return rg_nz_bits16(raw);
}

// ---- union-find in LDS (tile-local indices) -----------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(const volatile int* L, int a) {
    int p;
    while ((p = L[a]) != a) a = p;                 // strictly decreasing: at most `a` steps
    return a;
}
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
    bool done;
    do {                                           // every round that does not finish has lowered a label
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a < b) { const int old = atomicMin(&L[b], a); done = old == b; b = old; }
        else if (b < a) { const int old = atomicMin(&L[a], b); done = old == a; a = old; }
        else done = true;
    } while (!done);
}
// ---- union-find on the label array of one mask (pixel indices), device scope ------------------------------------------------
__device__ __forceinline__ int glb_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int glb_find(const int* L, int a) {
    int p;
    while ((p = glb_load(L + a)) != a) a = p;
    return a;
}
__device__ __forceinline__ void glb_union(int* L, int a, int b) {
    bool done;
    do {
        a = glb_find(L, a);
        b = glb_find(L, b);
        if (a < b) { const int old = atomicMin(&L[b], a); done = old == b; b = old; }
        else if (b < a) { const int old = atomicMin(&L[a], b); done = old == a; a = old; }
        else done = true;
    } while (!done);
}

// tile / segment of a thread.  grid (tiles_x * tiles_y, n), 256 threads
struct Seg { int m, y, x, ty0, tx0; bool in; };
__device__ __forceinline__ Seg rg_seg(int h, int w, int tiles_x) {
    Seg s;
    s.m = blockIdx.y;
    s.ty0 = ((int)blockIdx.x / tiles_x) * RG_TH;
    s.tx0 = ((int)blockIdx.x % tiles_x) * RG_TW;
    s.y = s.ty0 + ((int)threadIdx.x / RG_SEGS);
    s.x = s.tx0 + ((int)threadIdx.x % RG_SEGS) * 16;
    s.in = s.y < h && s.x < w;
    return s;
}

// 1. tile-local labels.  complement: the working set is the unset pixels (holes) instead of the set ones (islands).
// labels [n][h][w]: smallest pixel index (within the mask) of the pixel's tile-local component, -1 outside the working set.
// areas (or null): zeroed at every tile-local root, which is every index region_area_kernel can add to.
template <bool VEC>
__global__ __launch_bounds__(256) void region_local_kernel(const uint8_t* __restrict__ masks, int* __restrict__ labels,
                                                           int* __restrict__ areas, int h, int w, int tiles_x, int complement) {
    __shared__ __attribute__((aligned(16))) int lab[RG_TH * RG_TW];
    __shared__ uint32_t wbits[256];
    const Seg sg = rg_seg(h, w, tiles_x);
    const size_t mbase = (size_t)sg.m * h * w;
    const int t = threadIdx.x, ly = t / RG_SEGS, seg = t % RG_SEGS;
    uint32_t work = 0, valid = 0;
    if (sg.in) {
        uint32_t raw[4];
        const uint32_t set = rg_load_bits<VEC>(masks + mbase + (size_t)sg.y * w, sg.x, w, &valid, raw);
        work = (complement ? ~set : set) & valid;
    }
    const int any_work = __syncthreads_or(work != 0);
    const int any_rest = __syncthreads_or(work != valid);
    int out[16];
    if (!any_work || !any_rest) {                  // uniform tile: no iteration
        const int root = any_work ? sg.ty0 * w + sg.tx0 : -1;
#pragma unroll
        for (int i = 0; i < 16; ++i) out[i] = root;
        if (any_work && areas && t == 0) areas[mbase + root] = 0;
    } else {
        const int p0 = t * 16;                     // tile-local index of the segment's first pixel (row ly, column 16 seg)
        // a horizontal run inside the segment starts out labelled with its first pixel
        int cur = -1;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if ((work >> i) & 1u) { if (cur < 0) cur = p0 + i; } else cur = -1;
            out[i] = cur;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            *reinterpret_cast<int4*>(&lab[p0 + 4 * k]) = make_int4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
        wbits[t] = work;
        __syncthreads();
        // bit j = i + 1 of `row` / `up`: pixel i of this segment in this row / the row above; bits 0 and 17 are the neighbours' edges
        uint32_t row = work << 1, up = 0;
        if (seg > 0) row |= (wbits[t - 1] >> 15) & 1u;
        if (ly > 0) {
            up = wbits[t - RG_SEGS] << 1;
            if (seg > 0) up |= (wbits[t - RG_SEGS - 1] >> 15) & 1u;
            if (seg < RG_SEGS - 1) up |= (wbits[t - RG_SEGS + 1] & 1u) << 17;
        }
        // the unions that are not implied by others: W only at a segment start; N unless W and NW are both in (W made the link);
        // without N: NW unless W is in (W's N is that pixel), and NE
        // as bit masks over the segment's 16 pixels, so that the interior of a blob (W, NW and N all in) costs no iteration at all
        const uint32_t mW = row & 0xFFFFu, mNW = up & 0xFFFFu, mN = (up >> 1) & 0xFFFFu, mNE = (up >> 2) & 0xFFFFu;
        const uint32_t uW = work & mW & 1u, uN = work & mN & ~(mW & mNW), uNW = work & ~mN & mNW & ~mW, uNE = work & ~mN & mNE;
        for (uint32_t todo = uW | uN | uNW | uNE; todo; todo &= todo - 1) {
            const int i = __ffs((int)todo) - 1, p = p0 + i;
            if ((uW >> i) & 1u) lds_union(lab, p, p - 1);
            if ((uN >> i) & 1u) lds_union(lab, p, p - RG_TW);
            if ((uNW >> i) & 1u) lds_union(lab, p, p - RG_TW - 1);
            if ((uNE >> i) & 1u) lds_union(lab, p, p - RG_TW + 1);
        }
        __syncthreads();
        // one find per run of the segment, from the run's first pixel (out[] still holds it; the other pixels of a run were never
        // roots, so their entry still names it), and the chain it walked is cut short for the finds that follow: a component that
        // fills the tile hangs together row start by row start, 32 deep
        int last_s = -1, last_g = -1;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (!((work >> i) & 1u)) { out[i] = -1; continue; }
            const int s0 = out[i];
            if (s0 != last_s) {
                const int r = lds_find(lab, s0);
                if (r != s0) reinterpret_cast<volatile int*>(lab)[s0] = r;     // nothing unites any more: r is final
                last_s = s0;
                last_g = (sg.ty0 + r / RG_TW) * w + sg.tx0 + r % RG_TW;
                if (r == s0 && areas) areas[mbase + last_g] = 0;
            }
            out[i] = last_g;
        }
    }
    if (!sg.in) return;
    int* dst = labels + mbase + (size_t)sg.y * w + sg.x;
    if (VEC) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            reinterpret_cast<int4*>(dst)[k] = make_int4(out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if ((valid >> i) & 1u) dst[i] = out[i];
    }
}

// 2. unions across the tile borders.  Thread k < n_hor: pixel (y, x) on the first row of a tile row (y = RG_TH (1 + k / w),
// x = k % w), neighbours N, NW, NE; else pixel on the first column of a tile column (x = RG_TW (1 + k' / h), y = k' % h),
// neighbours W, NW, SW.  Links that others imply are left out as in region_local_kernel.  grid (blocks, n).
__global__ __launch_bounds__(256) void region_merge_kernel(int* __restrict__ labels, int h, int w, long long n_hor, long long n_all) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_all) return;
    int* L = labels + (size_t)blockIdx.y * h * w;
    if (k < n_hor) {
        const int y = RG_TH * (1 + (int)(k / w)), x = (int)(k % w);
        const int p = y * w + x;
        if (L[p] < 0) return;
        const int* up = L + p - w;
        const bool W = x > 0 && L[p - 1] >= 0, NW = x > 0 && up[-1] >= 0, N = up[0] >= 0, NE = x + 1 < w && up[1] >= 0;
        if (N) { if (!(W && NW)) glb_union(L, p, p - w); }
        else {
            if (NW && !W) glb_union(L, p, p - w - 1);
            if (NE) glb_union(L, p, p - w + 1);
        }
    } else {
        const long long kv = k - n_hor;
        const int x = RG_TW * (1 + (int)(kv / h)), y = (int)(kv % h);
        const int p = y * w + x;
        if (L[p] < 0) return;
        if (L[p - 1] >= 0) glb_union(L, p, p - 1);                 // NW and SW hang on W inside the left tile (or by a row link)
        else {
            if (y > 0 && L[p - w - 1] >= 0) glb_union(L, p, p - w - 1);
            if (y + 1 < h && L[p + w - 1] >= 0) glb_union(L, p, p + w - 1);
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void rg_load_labels(const int* __restrict__ src, uint32_t valid, int l[16]) {
    if (VEC) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int4 q = reinterpret_cast<const int4*>(src)[k];
            l[4 * k] = q.x; l[4 * k + 1] = q.y; l[4 * k + 2] = q.z; l[4 * k + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) l[i] = ((valid >> i) & 1u) ? src[i] : -1;
    }
}
__device__ __forceinline__ int rg_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// 3. the label each pixel holds (its tile-local root) -> re-pointed at the global root, and areas (or areas == null: the
// re-pointing alone; nothing unites any more, so a root that is read is final).  A thread's 16 pixels fall into at most
// 8 runs of one root each (two adjacent pixels of the working set share a component); the lanes of a wave offer their j-th run
// together, the lanes whose root matches the first offering lane's are summed on chip and added with one atomic, twice, and what
// still differs after that goes out on its own.
template <bool VEC>
__global__ __launch_bounds__(256) void region_area_kernel(int* labels, int* __restrict__ areas, int h, int w, int tiles_x) {
    const Seg sg = rg_seg(h, w, tiles_x);
    int* L = labels + (size_t)sg.m * h * w;
    int rr[8], rn[8], nr = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) { rr[j] = -1; rn[j] = 0; }
    if (sg.in) {
        const int p0 = sg.y * w + sg.x;
        const uint32_t valid = VEC ? 0xFFFFu : (1u << (w - sg.x < 16 ? w - sg.x : 16)) - 1u;
        int l[16];
        rg_load_labels<VEC>(L + p0, valid, l);
        int last_l = -1, last_r = -1;
        bool open = false;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (l[i] < 0) { open = false; continue; }
            if (l[i] != last_l) {
                last_l = l[i];
                const int first = glb_load(L + last_l);
                int a = last_l;
                last_r = first;
                while (last_r != a) { a = last_r; last_r = glb_load(L + a); }
                // the label this pixel holds now points at its root.  Other workgroups read this word with glb_load while it is
                // written (every writer stores the same final root, a reader is right with the old or the new value): an atomic store
                if (first != last_r) __hip_atomic_store(L + last_l, last_r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (open) {
#pragma unroll
                for (int j = 0; j < 8; ++j) if (j == nr - 1) rn[j] += 1;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) if (j == nr) { rr[j] = last_r; rn[j] = 1; }
                ++nr; open = true;
            }
        }
    }
    if (!areas) return;
    int* A = areas + (size_t)sg.m * h * w;
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (!__any(j < nr)) break;
        int r = rr[j];
        const int n = rn[j];
        for (int round = 0; round < 2; ++round) {
            const unsigned long long offer = __ballot(r >= 0);
            if (!offer) break;
            const int lead = __ffsll((long long)offer) - 1;
            const int lr = __shfl(r, lead, 64);
            const bool mine = r == lr;
            const int s = rg_wave_sum(mine ? n : 0);
            if (lane == lead) atomicAdd(&A[lr], s);
            if (mine) r = -1;
        }
        if (r >= 0) atomicAdd(&A[r], n);
    }
}

// 4. per mask: any component >= T, and the largest (first in row-major order among equals)
template <bool VEC>
__device__ __forceinline__ unsigned long long rg_best_key(const int* __restrict__ labels, const int* __restrict__ areas, const Seg& sg,
                                                          int w, int h) {
    const size_t mbase = (size_t)sg.m * h * w;
    const int p0 = sg.y * w + sg.x;
    const uint32_t valid = VEC ? 0xFFFFu : (1u << (w - sg.x < 16 ? w - sg.x : 16)) - 1u;
    int l[16];
    rg_load_labels<VEC>(labels + mbase + p0, valid, l);
    // the thread's best key first, then the wave's, and one atomic per wave -- and only where it can still raise the mask's key
    unsigned long long key = 0ull;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (l[i] != p0 + i) continue;                      // roots only
        const unsigned long long k = ((unsigned long long)(uint32_t)areas[mbase + p0 + i] << 32) | (0xFFFFFFFFu - (uint32_t)(p0 + i));
        key = k > key ? k : key;
    }
    return key;
}
template <bool VEC>
__global__ __launch_bounds__(256) void region_reduce_kernel(const int* __restrict__ labels, const int* __restrict__ areas, int h, int w,
                                                            int tiles_x, int T, RegionCtr* ctr) {
    const Seg sg = rg_seg(h, w, tiles_x);
    unsigned long long key = sg.in ? rg_best_key<VEC>(labels, areas, sg, w, h) : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) != 0 || key == 0ull) return;
    if ((int)(key >> 32) >= T) ctr[sg.m].any_big = 1u;
    if (key > __hip_atomic_load(&ctr[sg.m].best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&ctr[sg.m].best, key);
}

// 5. the mask in place.  complement (holes): a pixel of a small component becomes `fill` (1; or 2 in the first pass of BOTH, so
// that the second pass still knows what the input was).  Else (islands): 1 for what stays, 0 for the rest.  count: the counters
// take this pass's result; orig_one: a pixel counted as set in the INPUT only where its byte is 1 (second pass of BOTH).
template <bool VEC>
__global__ __launch_bounds__(256) void region_apply_kernel(uint8_t* __restrict__ masks, const int* __restrict__ labels,
                                                           const int* __restrict__ areas, int h, int w, int tiles_x, int T,
                                                           int complement, int fill, int count, int orig_one,
                                                           RegionCtr* __restrict__ ctr) {
    const Seg sg = rg_seg(h, w, tiles_x);
    int n_set = 0, n_chg = 0;
    if (sg.in) {
        const size_t mbase = (size_t)sg.m * h * w;
        const int p0 = sg.y * w + sg.x;
        uint8_t* row = masks + mbase + (size_t)sg.y * w;
        uint32_t valid, raw[4];
        const uint32_t set_in = rg_load_bits<VEC>(row, sg.x, w, &valid, raw);
        int l[16];
        rg_load_labels<VEC>(labels + mbase + p0, valid, l);
        const int* L = labels + mbase;
        const int* A = areas + mbase;
        bool all_small = false;
        int keep_root = -1;
        if (!complement) {
            all_small = ctr[sg.m].any_big == 0u;
            keep_root = (int)(0xFFFFFFFFu - (uint32_t)(ctr[sg.m].best & 0xFFFFFFFFull));
        }
        uint32_t out[4] = {0u, 0u, 0u, 0u};
        uint32_t orig = set_in;
        if (orig_one) {
            orig = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) orig |= (uint32_t)(((raw[i >> 2] >> (8 * (i & 3))) & 0xFFu) == 1u) << i;
        }
        int last_l = -1, last_v = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (!((valid >> i) & 1u)) continue;
            int v;
            if (l[i] < 0) v = complement ? 1 : 0;          // outside the working set: set pixels stay (holes), unset stay (islands)
            else {
                if (l[i] != last_l) {
                    last_l = l[i];
                    const int r = L[l[i]];                 // two loads reach the root (region_area_kernel)
                    const bool small = A[r] < T;
                    if (complement) last_v = small ? fill : 0;
                    else last_v = all_small ? (r == keep_root) : !small;
                }
                v = last_v;
            }
            out[i >> 2] |= (uint32_t)v << (8 * (i & 3));
            n_set += v != 0;
            n_chg += (v != 0) != (bool)((orig >> i) & 1u);
        }
        if (out[0] != raw[0] || out[1] != raw[1] || out[2] != raw[2] || out[3] != raw[3]) {
            if (VEC) *reinterpret_cast<uint4*>(row + sg.x) = make_uint4(out[0], out[1], out[2], out[3]);
            else {
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if ((valid >> i) & 1u) row[sg.x + i] = (uint8_t)(out[i >> 2] >> (8 * (i & 3)));
            }
        }
    }
    if (!count) return;
    n_set = rg_wave_sum(n_set);
    n_chg = rg_wave_sum(n_chg);
    if ((threadIdx.x & 63) == 0) {
        if (n_set) atomicAdd(&ctr[sg.m].set, (unsigned long long)n_set);
        if (n_chg) atomicAdd(&ctr[sg.m].changed, (unsigned long long)n_chg);
    }
}

__global__ void region_counts_kernel(const RegionCtr* __restrict__ ctr, int n, long long* __restrict__ areas_out,
                                     long long* __restrict__ changed_out) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n) return;
    if (areas_out) areas_out[m] = (long long)ctr[m].set;
    if (changed_out) changed_out[m] = (long long)ctr[m].changed;
}

// samrs_k_region_labels: out[p] = root(p) = L[L[p]], in place (an entry that other pixels point at already holds the root)
__global__ __launch_bounds__(256) void region_flatten_kernel(int* __restrict__ labels, long long hw) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    int* L = labels + (size_t)blockIdx.y * hw;
    const int l = L[p];
    if (l >= 0 && l != p) L[p] = L[l];
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// local + merge + (re-point, areas) of one working set
hipError_t region_label(const uint8_t* masks, int n, int h, int w, int complement, int* labels, int* areas, bool vec, hipStream_t s) {
    const int tiles_x = (w + RG_TW - 1) / RG_TW, tiles_y = (h + RG_TH - 1) / RG_TH;
    const dim3 grid((unsigned)(tiles_x * tiles_y), n);
    if (vec) region_local_kernel<true><<<grid, 256, 0, s>>>(masks, labels, areas, h, w, tiles_x, complement);
    else region_local_kernel<false><<<grid, 256, 0, s>>>(masks, labels, areas, h, w, tiles_x, complement);
    const long long n_hor = (long long)(tiles_y - 1) * w, n_all = n_hor + (long long)(tiles_x - 1) * h;
    if (n_all > 0) region_merge_kernel<<<dim3((unsigned)((n_all + 255) / 256), n), 256, 0, s>>>(labels, h, w, n_hor, n_all);
    if (vec) region_area_kernel<true><<<grid, 256, 0, s>>>(labels, areas, h, w, tiles_x);
    else region_area_kernel<false><<<grid, 256, 0, s>>>(labels, areas, h, w, tiles_x);
    return hipGetLastError();
}

}  // namespace

size_t region_scratch_bytes(int n, int h, int w) {
    return 2 * align256((size_t)n * h * w * sizeof(int)) + align256((size_t)n * sizeof(RegionCtr));
}

hipError_t launch_region_labels(const uint8_t* masks, int n, int h, int w, int complement, int32_t* labels_out, hipStream_t s) {
    if (!masks || !labels_out || n < 1 || h < 1 || w < 1 || (size_t)h * w >= (1ull << 30)) return hipErrorInvalidValue;
    const size_t hw = (size_t)h * w;
    for (int off = 0; off < n; off += REGION_CHUNK) {
        const int m = n - off < REGION_CHUNK ? n - off : REGION_CHUNK;
        const uint8_t* src = masks + (size_t)off * hw;
        int* L = labels_out + (size_t)off * hw;
        const bool vec = (w & 15) == 0 && (((uintptr_t)src) & 15) == 0 && (((uintptr_t)L) & 15) == 0;
        HIP_CHECK_RET(region_label(src, m, h, w, complement != 0, L, nullptr, vec, s));
        region_flatten_kernel<<<dim3((unsigned)((hw + 255) / 256), m), 256, 0, s>>>(L, (long long)hw);
    }
    return hipGetLastError();
}

hipError_t launch_clean_masks(uint8_t* masks, int n, int h, int w, int min_area, int mode, void* scratch, long long* areas_out,
                              long long* changed_out, hipStream_t s) {
    if (!masks || !scratch || n < 1 || n > REGION_CHUNK || h < 1 || w < 1 || min_area < 1 || mode < 1 || mode > 3 ||
        (size_t)h * w >= (1ull << 30))
        return hipErrorInvalidValue;
    const size_t lab_bytes = align256((size_t)n * h * w * sizeof(int));
    unsigned char* p = reinterpret_cast<unsigned char*>(scratch);
    int* labels = reinterpret_cast<int*>(p);
    int* areas = reinterpret_cast<int*>(p + lab_bytes);
    RegionCtr* ctr = reinterpret_cast<RegionCtr*>(p + 2 * lab_bytes);
    const bool vec = (w & 15) == 0 && (((uintptr_t)masks) & 15) == 0;
    const int tiles_x = (w + RG_TW - 1) / RG_TW, tiles_y = (h + RG_TH - 1) / RG_TH;
    const dim3 grid((unsigned)(tiles_x * tiles_y), n);
    for (int pass = 1; pass <= 2; ++pass) {               // 1 = holes, 2 = islands
        if (!(mode & pass)) continue;
        const int complement = pass == 1;
        const int last = pass == 2 || mode == 1;
        const int fill = last ? 1 : 2, orig_one = pass == 2 && mode == 3;
        HIP_CHECK_RET(hipMemsetAsync(ctr, 0, (size_t)n * sizeof(RegionCtr), s));
        HIP_CHECK_RET(region_label(masks, n, h, w, complement, labels, areas, vec, s));
        if (!complement) {
            if (vec) region_reduce_kernel<true><<<grid, 256, 0, s>>>(labels, areas, h, w, tiles_x, min_area, ctr);
            else region_reduce_kernel<false><<<grid, 256, 0, s>>>(labels, areas, h, w, tiles_x, min_area, ctr);
        }
        if (vec) region_apply_kernel<true><<<grid, 256, 0, s>>>(masks, labels, areas, h, w, tiles_x, min_area, complement, fill, last, orig_one, ctr);
        else region_apply_kernel<false><<<grid, 256, 0, s>>>(masks, labels, areas, h, w, tiles_x, min_area, complement, fill, last, orig_one, ctr);
    }
    if (areas_out || changed_out) region_counts_kernel<<<(n + 63) / 64, 64, 0, s>>>(ctr, n, areas_out, changed_out);
    return hipGetLastError();
}
