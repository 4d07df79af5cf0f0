// box_kernels.hip -- boxes derived from full-resolution binary masks on the device (gfx950): the tight horizontal box and the
// minimum-area rotated box of every mask of a batch that never leaves HBM.
//
// Definition (tests/box_ref.py restates it in numpy and Python integers; tests/test_mask_boxes_gpu.py asks for exact equality):
//   points      the set pixels of a mask as integer points (x0 + col, y0 + row): pixel CENTRES, the convention of
//               cv2.findContours -> cv2.minAreaRect and the frame the reference's rbox polygons are stated in;
//   hbox        (xmin, ymin, xmax, ymax), inclusive integers;
//   hull        the strict vertices of the convex hull (no collinear points), from v0 = the set pixel with the smallest (y, x): down
//               the left side to the leftmost pixel of the last non-empty row, along that row to its rightmost pixel, up the right
//               side to the rightmost pixel of the first non-empty row, back to v0; a repeated point appears once.  m vertices
//               (1 for one pixel, 2 for collinear pixels);
//   candidates  edge k runs from vertex k to vertex (k + 1) mod m; (dx, dy) = v[k + 1] - v[k], not reduced by the gcd.  Over the
//               hull vertices p = x dx + y dy, q = -x dy + y dx; the candidate's rectangle has area
//               (pmax - pmin)(qmax - qmin) / (dx^2 + dy^2), an exact rational;
//   winner      the smallest area, compared exactly (cross-multiplied, up to 2^81: unsigned __int128); ties go to the smallest k.
//               m = 1: (dx, dy) = (1, 0);
//   corners     (pmin, qmin), (pmax, qmin), (pmax, qmax), (pmin, qmax) with x = (p dx - q dy) / L, y = (p dy + q dx) / L,
//               L = dx^2 + dy^2: the integer numerator (below 2^53) converted to fp64, divided once (IEEE, correctly rounded: this
//               library is built without fast-math or reciprocal division), rounded to fp32;
//   record      int64 [8]: dx, dy, pmin, pmax, qmin, qmax, m, and twice the hull's area = sum over the ordered vertices of
//               x[k + 1] y[k] - x[k] y[k + 1] (>= 0 in this order);
//   empty mask  m = 0 and every output of that mask is zero.
// Not pinned against cv2 itself: cv2.minAreaRect works from the same hull, so it can differ only in float rounding and in which
// of several equal-area rectangles it returns.
//
// Two launches on the caller's stream:
//   1. mask_row_extents_kernel  one wave per (mask, row): every mask byte is read once (16-byte loads where w % 16 == 0 and the
//                               base is 16-byte aligned, byte loads otherwise), wave-level min / max / add -> first set column,
//                               last set column, pixel count of the row (-1, -1, 0 for an empty row), int32 [n][h][3].
//   2. mask_hull_rect_kernel    one workgroup per mask: the non-empty rows' (y, lo, hi) compacted into LDS (6 bytes per row), the
//                               hbox reduced, the strict vertices of the left chain (convex minorant of lo over y) and of the right
//                               chain (concave majorant of hi over y) marked -- point i is a vertex iff the largest slope from any
//                               earlier point to i is strictly below (right chain: the smallest strictly above) the smallest
//                               (largest) slope from i to any later point; one thread per point, the other points broadcast reads
//                               from LDS, fractions compared by cross-multiplication --, compacted in the order above, every
//                               candidate edge evaluated against every vertex from LDS, block-wide argmin with the exact comparison.
// Integer arithmetic only up to the one division per corner coordinate.  A chain over h, w <= 8192 has at most 715 edges (distinct
// primitive directions with dy >= 1 whose |dx| + dy sum to at most 16382), so BX_VCAP vertices always suffice.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int BX_THREADS = 1024;                   // mask_hull_rect_kernel: 16 waves
constexpr int BX_WAVES = BX_THREADS / 64;
constexpr int BX_VCAP = 2048;                      // hull vertices kept in LDS (<= 2 * 716 by the bound above)

__device__ __forceinline__ uint32_t bx_nz_bytes(uint32_t w) {      // 0x80 in every byte of w that is not 0
    return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;
}
// bit i = byte i of the 16 bytes is not 0
__device__ __forceinline__ uint32_t bx_nz_bits16(const uint4 q) {
    const uint32_t v[4] = {q.x, q.y, q.z, q.w};
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t t = bx_nz_bytes(v[k]) >> 7;                 // 0x01 per non-zero byte
        bits |= ((t & 1u) | ((t >> 7) & 2u) | ((t >> 14) & 4u) | ((t >> 21) & 8u)) << (4 * k);
    }
    return bits;
}

// 1. rows = n * h rows of w bytes; wave r of the grid owns row r.  VEC: w % 16 == 0 and a 16-byte aligned base (launcher).
template <bool VEC>
__global__ __launch_bounds__(256) void mask_row_extents_kernel(const uint8_t* __restrict__ masks, long long rows, int w,
                                                               int32_t* __restrict__ ext) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                         // uniform over the wave
    const int lane = threadIdx.x & 63;
    const uint8_t* __restrict__ row = masks + (size_t)r * w;
    int lo = 0x7fffffff, hi = -1, cnt = 0;
    for (int x = lane * 16; x < w; x += 64 * 16) {
        uint32_t bits = 0;
        if (VEC) bits = bx_nz_bits16(*reinterpret_cast<const uint4*>(row + x));
        else {
            const int nv = w - x < 16 ? w - x : 16;
            for (int i = 0; i < nv; ++i) bits |= (uint32_t)(row[x + i] != 0) << i;
        }
        if (bits) {
            const int f = x + __ffs((int)bits) - 1, l = x + 31 - __clz((int)bits);
            lo = f < lo ? f : lo;
            hi = l > hi ? l : hi;
            cnt += __popc(bits);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int a = __shfl_xor(lo, off, 64), b = __shfl_xor(hi, off, 64);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
        cnt += __shfl_xor(cnt, off, 64);
    }
    if (lane == 0) {
        int32_t* o = ext + r * 3;
        o[0] = cnt ? lo : -1;
        o[1] = hi;
        o[2] = cnt;
    }
}

// exclusive prefix of `flag` over the block's threads (thread order) and the block's total; wsum: LDS int [BX_WAVES]
__device__ __forceinline__ int bx_scan(bool flag, int* wsum, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < BX_WAVES; ++i) {
        const int v = wsum[i];
        base += i < wave ? v : 0;
        tot += v;
    }
    __syncthreads();                                               // wsum is free again
    *total = tot;
    return base + __popcll(b & ((1ull << lane) - 1ull));
}

__device__ __forceinline__ long long bx_block_sum(long long v, long long* wll) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) wll[threadIdx.x >> 6] = v;
    __syncthreads();
    long long s = 0;
#pragma unroll
    for (int i = 0; i < BX_WAVES; ++i) s += wll[i];
    __syncthreads();
    return s;
}

// a candidate: area N / L of edge k (k < 0: none).  a before b: the smaller area, then the smaller k
struct BxCand { unsigned long long N; unsigned int L; int k; };
__device__ __forceinline__ bool bx_before(const BxCand& a, const BxCand& b) {
    if (a.k < 0) return false;
    if (b.k < 0) return true;
    const unsigned __int128 l = (unsigned __int128)a.N * b.L, r = (unsigned __int128)b.N * a.L;
    return l < r || (l == r && a.k < b.k);
}

// 2. grid n, BX_THREADS threads, dynamic LDS bx_lds_bytes(h).  ext: int32 [n][h][3] of kernel 1.  Every output may be null.
__global__ __launch_bounds__(BX_THREADS) void mask_hull_rect_kernel(const int32_t* __restrict__ ext, int h, int x0, int y0,
                                                                    int32_t* __restrict__ hbox_out, float* __restrict__ rbox_out,
                                                                    long long* __restrict__ rec_out, int32_t* __restrict__ verts_out,
                                                                    int cap, int32_t* __restrict__ counts_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bx_smem[];
    long long* wll = reinterpret_cast<long long*>(bx_smem);                    // [BX_WAVES]
    unsigned long long* candN = reinterpret_cast<unsigned long long*>(wll + BX_WAVES);   // [BX_WAVES]
    unsigned int* candL = reinterpret_cast<unsigned int*>(candN + BX_WAVES);   // [BX_WAVES]
    int* candK = reinterpret_cast<int*>(candL + BX_WAVES);                     // [BX_WAVES]
    int* wsum = candK + BX_WAVES;                                              // [BX_WAVES]
    int* wmin = wsum + BX_WAVES;                                               // [BX_WAVES]
    int* wmax = wmin + BX_WAVES;                                               // [BX_WAVES]
    const int hp = (h + 7) & ~7;
    uint16_t* ry = reinterpret_cast<uint16_t*>(wmax + BX_WAVES);               // [hp] row of the i-th non-empty row
    uint16_t* rlo = ry + hp;                                                   // [hp] its first set column
    uint16_t* rhi = rlo + hp;                                                  // [hp] its last set column
    uint16_t* vx = rhi + hp;                                                   // [BX_VCAP] hull vertices, window frame
    uint16_t* vy = vx + BX_VCAP;
    const int mask = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* __restrict__ E = ext + (size_t)mask * h * 3;

    // the non-empty rows, in row order
    int R = 0, xmin = 0x7fffffff, xmax = -1;
    for (int yc = 0; yc < h; yc += BX_THREADS) {
        const int y = yc + tid;
        int lo = 0, hi = 0;
        bool f = false;
        if (y < h) {
            lo = E[3 * y];
            hi = E[3 * y + 1];
            f = E[3 * y + 2] > 0;
        }
        int tot;
        const int pos = R + bx_scan(f, wsum, &tot);
        if (f) {
            ry[pos] = (uint16_t)y; rlo[pos] = (uint16_t)lo; rhi[pos] = (uint16_t)hi;
            xmin = lo < xmin ? lo : xmin;
            xmax = hi > xmax ? hi : xmax;
        }
        R += tot;
    }
    if (R == 0) {                                                  // empty mask: every output is zero
        if (tid < 4 && hbox_out) hbox_out[(size_t)mask * 4 + tid] = 0;
        if (tid < 8) {
            if (rbox_out) rbox_out[(size_t)mask * 8 + tid] = 0.0f;
            if (rec_out) rec_out[(size_t)mask * 8 + tid] = 0;
        }
        if (tid == 0 && counts_out) counts_out[mask] = 0;
        return;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int a = __shfl_xor(xmin, off, 64), b = __shfl_xor(xmax, off, 64);
        xmin = a < xmin ? a : xmin;
        xmax = b > xmax ? b : xmax;
    }
    if (lane == 0) { wmin[wave] = xmin; wmax[wave] = xmax; }
    __syncthreads();                                               // also: ry / rlo / rhi are complete
    if (tid == 0 && hbox_out) {
        for (int i = 0; i < BX_WAVES; ++i) {
            xmin = wmin[i] < xmin ? wmin[i] : xmin;
            xmax = wmax[i] > xmax ? wmax[i] : xmax;
        }
        int32_t* o = hbox_out + (size_t)mask * 4;
        o[0] = x0 + xmin; o[1] = y0 + (int)ry[0]; o[2] = x0 + xmax; o[3] = y0 + (int)ry[R - 1];
    }

    // strict chain vertices: bit c of fl / fr = point c * BX_THREADS + tid is a vertex of the left / right chain (h <= 8192: c < 8)
    unsigned int fl = 0, fr = 0;
    for (int c = 0, i = tid; i < R; ++c, i += BX_THREADS) {
        bool vl = true, vr = true;                                 // the end points always are vertices
        if (i > 0 && i < R - 1) {
            const int yi = ry[i], li = rlo[i], hi = rhi[i];
            // slopes as fractions n / d with d > 0; |n|, d < 8192, so the cross products fit 32 bits
            int an = li - (int)rlo[i - 1], ad = yi - (int)ry[i - 1];           // left: largest slope from an earlier point
            int cn = hi - (int)rhi[i - 1], cd = ad;                            // right: smallest slope from an earlier point
            for (int j = 0; j < i - 1; ++j) {
                const int d = yi - (int)ry[j], nl = li - (int)rlo[j], nr = hi - (int)rhi[j];
                if (nl * ad > an * d) { an = nl; ad = d; }
                if (nr * cd < cn * d) { cn = nr; cd = d; }
            }
            int bn = (int)rlo[i + 1] - li, bd = (int)ry[i + 1] - yi;           // left: smallest slope to a later point
            int dn = (int)rhi[i + 1] - hi, dd = bd;                            // right: largest slope to a later point
            for (int k = i + 2; k < R; ++k) {
                const int d = (int)ry[k] - yi, nl = (int)rlo[k] - li, nr = (int)rhi[k] - hi;
                if (nl * bd < bn * d) { bn = nl; bd = d; }
                if (nr * dd > dn * d) { dn = nr; dd = d; }
            }
            vl = an * bd < bn * ad;
            vr = cn * dd > dn * cd;
        }
        fl |= (unsigned int)vl << c;
        fr |= (unsigned int)vr << c;
    }
    // right-chain vertices in all (they are placed in falling row order)
    const int mR = (int)bx_block_sum((long long)__popc(fr), wll);
    // a repeated point appears once: the last row's two ends, the first row's two ends
    const int skip_first = rlo[R - 1] == rhi[R - 1] ? 1 : 0;
    const int skip_last = (R > 1 && rlo[0] == rhi[0]) ? 1 : 0;
    int mL = 0, nR = 0;
    for (int c = 0, ic = 0; ic < R; ++c, ic += BX_THREADS) {       // the left chain, in rising row order
        const int i = ic + tid;
        const bool vl = (fl >> c) & 1u;
        int tot;
        const int pl = mL + bx_scan(vl, wsum, &tot);
        mL += tot;
        if (vl && pl < BX_VCAP) { vx[pl] = rlo[i]; vy[pl] = ry[i]; }
    }
    for (int c = 0, ic = 0; ic < R; ++c, ic += BX_THREADS) {       // the right chain behind it, in falling row order
        const int i = ic + tid;
        const bool vr = (fr >> c) & 1u;
        int tot;
        const int pr = nR + bx_scan(vr, wsum, &tot);
        nR += tot;
        if (vr) {
            const int rr = mR - 1 - pr;                            // position in falling row order
            const int at = mL + rr - skip_first;
            if (!((rr == 0 && skip_first) || (rr == mR - 1 && skip_last)) && at < BX_VCAP) { vx[at] = rhi[i]; vy[at] = ry[i]; }
        }
    }
    int m = mL + mR - skip_first - skip_last;
    m = m < BX_VCAP ? m : BX_VCAP;
    __syncthreads();                                               // vx / vy are complete

    if (counts_out && tid == 0) counts_out[mask] = m;
    if (verts_out) {
        const int nv = m < cap ? m : cap;
        for (int k = tid; k < nv; k += BX_THREADS) {
            int32_t* o = verts_out + ((size_t)mask * cap + k) * 2;
            o[0] = x0 + (int)vx[k];
            o[1] = y0 + (int)vy[k];
        }
    }
    if (!rbox_out && !rec_out) return;                             // uniform

    // twice the hull's area, and every candidate edge against every vertex
    long long sh = 0;
    BxCand best = {0ull, 1u, -1};
    long long b_dx = 0, b_dy = 0, b_pmin = 0, b_pmax = 0, b_qmin = 0, b_qmax = 0;
    for (int k = tid; k < m; k += BX_THREADS) {
        const int k1 = k + 1 < m ? k + 1 : 0;
        const long long xa = x0 + (int)vx[k], ya = y0 + (int)vy[k], xb = x0 + (int)vx[k1], yb = y0 + (int)vy[k1];
        sh += xb * ya - xa * yb;
        const long long dx = m > 1 ? xb - xa : 1, dy = m > 1 ? yb - ya : 0;
        long long pmin = 0x7fffffffffffffffll, pmax = -0x7fffffffffffffffll, qmin = pmin, qmax = pmax;
        for (int j = 0; j < m; ++j) {
            const long long x = x0 + (int)vx[j], y = y0 + (int)vy[j];
            const long long p = x * dx + y * dy, q = y * dx - x * dy;
            pmin = p < pmin ? p : pmin; pmax = p > pmax ? p : pmax;
            qmin = q < qmin ? q : qmin; qmax = q > qmax ? q : qmax;
        }
        const BxCand c = {(unsigned long long)((pmax - pmin) * (qmax - qmin)), (unsigned int)(dx * dx + dy * dy), k};
        if (bx_before(c, best)) {
            best = c;
            b_dx = dx; b_dy = dy; b_pmin = pmin; b_pmax = pmax; b_qmin = qmin; b_qmax = qmax;
        }
    }
    const long long area2 = bx_block_sum(sh, wll);
    BxCand win = best;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        BxCand o;
        o.N = __shfl_xor(win.N, off, 64);
        o.L = __shfl_xor(win.L, off, 64);
        o.k = __shfl_xor(win.k, off, 64);
        if (bx_before(o, win)) win = o;
    }
    if (lane == 0) { candN[wave] = win.N; candL[wave] = win.L; candK[wave] = win.k; }
    __syncthreads();
    win.k = -1;
    for (int i = 0; i < BX_WAVES; ++i) {
        const BxCand o = {candN[i], candL[i], candK[i]};
        if (bx_before(o, win)) win = o;
    }
    if (best.k < 0 || best.k != win.k) return;                     // the thread that evaluated the winning edge writes
    if (rec_out) {
        long long* o = rec_out + (size_t)mask * 8;
        o[0] = b_dx; o[1] = b_dy; o[2] = b_pmin; o[3] = b_pmax; o[4] = b_qmin; o[5] = b_qmax; o[6] = m; o[7] = area2;
    }
    if (rbox_out) {
        float* o = rbox_out + (size_t)mask * 8;
        const double L = (double)(b_dx * b_dx + b_dy * b_dy);
        const long long ps[4] = {b_pmin, b_pmax, b_pmax, b_pmin}, qs[4] = {b_qmin, b_qmin, b_qmax, b_qmax};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            o[2 * c] = (float)((double)(ps[c] * b_dx - qs[c] * b_dy) / L);
            o[2 * c + 1] = (float)((double)(ps[c] * b_dy + qs[c] * b_dx) / L);
        }
    }
}

inline size_t bx_lds_bytes(int h) {
    const size_t hp = (size_t)((h + 7) & ~7);
    return BX_WAVES * (8 + 8 + 4 + 4 + 4 + 4 + 4) + 3 * hp * 2 + 2 * (size_t)BX_VCAP * 2;
}

}  // namespace

bool mask_boxes_shape_ok(int h, int w, int x0, int y0) {
    return h >= 1 && w >= 1 && h <= 8192 && w <= 8192 && x0 >= 0 && y0 >= 0 && x0 + w <= 32768 && y0 + h <= 32768;
}

size_t mask_boxes_scratch_bytes(int n, int h) { return (size_t)n * h * 3 * sizeof(int32_t); }

hipError_t launch_mask_row_extents(const uint8_t* masks, int n, int h, int w, int32_t* ext, hipStream_t s) {
    if (!masks || !ext || n < 1 || !mask_boxes_shape_ok(h, w, 0, 0)) return hipErrorInvalidValue;
    const long long rows = (long long)n * h;
    if ((rows + 3) / 4 > 0x7fffffffll) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((rows + 3) / 4);
    if ((w & 15) == 0 && (((uintptr_t)masks) & 15) == 0) mask_row_extents_kernel<true><<<blocks, 256, 0, s>>>(masks, rows, w, ext);
    else mask_row_extents_kernel<false><<<blocks, 256, 0, s>>>(masks, rows, w, ext);
    return hipGetLastError();
}

hipError_t launch_mask_hull_rect(const int32_t* ext, int n, int h, int x0, int y0, int32_t* hbox_out, float* rbox_out,
                                 long long* record_out, int32_t* verts_out, int cap, int32_t* counts_out, hipStream_t s) {
    if (!ext || n < 1 || !mask_boxes_shape_ok(h, 1, x0, y0) || (verts_out && cap < 1)) return hipErrorInvalidValue;
    mask_hull_rect_kernel<<<n, BX_THREADS, bx_lds_bytes(h), s>>>(ext, h, x0, y0, hbox_out, rbox_out, record_out, verts_out, cap,
                                                                 counts_out);
    return hipGetLastError();
}
