// polygon_kernels.hip -- the outlines of full-resolution binary masks as polygons on the device (gfx950): outer rings and holes of
// every mask of a batch that never leaves HBM.
//
// Definition (include/samrs_hip.h samrs_mask_polygons states the contract; tests/polygon_ref.py restates it in numpy and a plain
// sequential walk; tests/test_polygons_gpu.py asks for exact equality, stage by stage and end to end):
//   lattice     vertex (x, y), 0 <= x <= w, 0 <= y <= h, is the top-left CORNER of pixel (row y, col x) -- not the pixel centre of
//               box_kernels.hip;
//   crack edge  a unit lattice segment between a set pixel and an unset one (outside the image = unset), directed so that the set
//               pixel is on the right hand of travel (y down).  Set pixel p = y w + x owns id = 4 p + d: d = 0 top, heading E;
//               1 right, S; 2 bottom, W; 3 left, N;
//   successor   at the end vertex of P's edge d: L = the pixel ahead on the left, R = the pixel straight ahead.  L set: L's edge
//               (d + 3) % 4 (a saddle joins the diagonal pixels: 8-connected foreground); else R set: R's edge d; else P's edge
//               (d + 1) % 4.  A bijection: the edges fall into rings;
//   ring        leader = its smallest edge id (a top edge: outer ring, a bottom edge: hole), rank = distance from the leader along
//               the successor; a corner = an edge whose direction differs from its predecessor's; the polygon = the start vertices
//               of the corner edges in rank order.
// Per chunk of masks, on the caller's stream; every cross-workgroup dependence is a kernel boundary, integer arithmetic only:
//   1. pg_seg_bits_kernel     a lane owns 16 pixels of a row (a "segment"; 16-byte loads where w % 16 == 0 and the base is aligned,
//                             byte loads otherwise), reads rows y - 1, y, y + 1 -> the four 16-bit edge masks of the segment
//                             (S & ~S_above, S & ~S_right, ...) and their popcount;
//   2. pg_seg_scan_kernel     one workgroup per mask: exclusive scan of the counts -> the segment's first compact index (the compact
//                             list is in ascending id order, so a ring's leader is its smallest compact index), edges per mask;
//   3. pg_link_kernel         per segment: every edge's id, its successor's compact index (two pixel reads, then the target
//                             segment's offset + popcounts of its masks), its corner flag (mirror rule: two pixel reads);
//   4. pg_double_kernel       ceil(log2(edge cap)) rounds of pointer doubling on the uncut cycles, ping-pong: (jump, min, off) per
//                             edge; round k takes min[jump] when smaller with off = off[jump] + 2^k, then jump = jump[jump];
//   5. pg_rank_kernel         leader = min, ring length L = off[succ(leader)] + 1, rank = (L - off) % L;
//   6. pg_ring_scan_kernel    per mask: exclusive scan of L over the leaders in index order = ring base, ring ordinal, ring count;
//   7. pg_scatter_kernel      edge -> position base + rank: its start vertex when it is a corner, and its shoelace term;
//   8. pg_corner_scan_kernel  per mask: exclusive scan over the positions of (corner count, shoelace sum) in one 64-bit word;
//   9. pg_place_kernel        one thread walks the chunk's masks: cursor, capacity and edge-cap rules -> table;
//  10. pg_emit_kernel         vertices behind the cursor, ring records.
// Masks over the edge cap stop after 2.  No inline assembly, no scalar-memory instructions: vector stores and plain C++.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int PG_SCAN_THREADS = 1024;
constexpr int PG_SCAN_ITEMS = 4;                   // consecutive items per thread and tile of the per-mask scans
typedef unsigned long long pg_u64;

__device__ __forceinline__ uint32_t pg_nz_bytes(uint32_t w) {      // 0x80 in every byte of w that is not 0
    return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;
}
__device__ __forceinline__ uint32_t pg_nz_bits16(const uint4 q) {  // bit i = byte i of the 16 bytes is not 0
    const uint32_t v[4] = {q.x, q.y, q.z, q.w};
    uint32_t bits = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t t = pg_nz_bytes(v[k]) >> 7;
        bits |= ((t & 1u) | ((t >> 7) & 2u) | ((t >> 14) & 4u) | ((t >> 21) & 8u)) << (4 * k);
    }
    return bits;
}

// the 16 pixels x .. x + 15 of a row as bits (pixels at or beyond w: 0)
template <bool VEC>
__device__ __forceinline__ uint32_t pg_row_bits(const uint8_t* __restrict__ row, int x, int w) {
    if (VEC) return pg_nz_bits16(*reinterpret_cast<const uint4*>(row + x));
    uint32_t bits = 0;
    const int nv = w - x < 16 ? w - x : 16;
    for (int i = 0; i < nv; ++i) bits |= (uint32_t)(row[x + i] != 0) << i;
    return bits;
}

// the scratch of one chunk: per mask, seg* hold NS = h * ceil(w / 16) entries, the edge arrays ecap (+ 1) entries
struct PgScratch {
    uint2* segbits;        // x = top | right << 16, y = bottom | left << 16 (bit i = pixel i of the segment has that edge)
    uint32_t* segoff;      // edges of the segment, then (scan) the compact index of its first edge
    uint32_t* eid;         // edge id 4 p + d, ascending
    int32_t* succ;         // compact index of the successor
    uint8_t* corner;       // 1: the direction differs from the predecessor's
    int4* stA;             // (jump, min, off, -) ping
    int4* stB;             // pong
    int32_t* lead;         // compact index of the ring's leader
    int32_t* rank;         // distance from the leader along the successor
    pg_u64* lr;            // [ecap + 1] leader ? 1 << 32 | L : 0, then its exclusive scan (ring ordinal << 32 | ring base)
    int32_t* pvert;        // [position] y << 16 | x of the start vertex when the edge there is a corner, else -1
    pg_u64* cs;            // [ecap + 1] shoelace term << 32 | corner, then its exclusive scan
    int32_t* totals;       // [n][4] edges, rings, vertices, -
    long long* placed;     // [n][2] first ring, first vertex (absolute), -1: not placed
    size_t ns;             // segments per mask
    size_t ecap;           // edge capacity per mask
};

// 1. grid (ceil(NS / 256), n): thread = segment
template <bool VEC>
__global__ __launch_bounds__(256) void pg_seg_bits_kernel(const uint8_t* __restrict__ masks, int h, int w, int sr, PgScratch sc) {
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= sc.ns) return;
    const int m = blockIdx.y, y = (int)(s / sr), x = (int)(s % sr) * 16;
    const uint8_t* __restrict__ row = masks + ((size_t)m * h + y) * w;
    const uint32_t S = pg_row_bits<VEC>(row, x, w);
    uint32_t T = 0, R = 0, B = 0, L = 0;
    if (S) {
        const uint32_t A = y > 0 ? pg_row_bits<VEC>(row - w, x, w) : 0u;
        const uint32_t Bl = y + 1 < h ? pg_row_bits<VEC>(row + w, x, w) : 0u;
        const uint32_t lb = x > 0 ? (uint32_t)(row[x - 1] != 0) : 0u;
        const uint32_t rb = x + 16 < w ? (uint32_t)(row[x + 16] != 0) : 0u;
        T = S & ~A;
        B = S & ~Bl;
        L = S & ~((S << 1) | lb) & 0xffffu;
        R = S & ~((S >> 1) | (rb << 15));
    }
    sc.segbits[(size_t)m * sc.ns + s] = make_uint2(T | (R << 16), B | (L << 16));
    sc.segoff[(size_t)m * sc.ns + s] = __popc(T) + __popc(R) + __popc(B) + __popc(L);
}

// exclusive scan, by the whole block (PG_SCAN_THREADS threads), of load(k), k < count, 64-bit wrapping sums; store(k, exclusive
// prefix); returns the total.  sm: LDS pg_u64 [17].
template <class Load, class Store>
__device__ __forceinline__ pg_u64 pg_block_scan(size_t count, Load load, Store store, pg_u64* sm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    pg_u64 run = 0;
    for (size_t t0 = 0; t0 < count; t0 += (size_t)PG_SCAN_THREADS * PG_SCAN_ITEMS) {
        const size_t k0 = t0 + (size_t)threadIdx.x * PG_SCAN_ITEMS;
        pg_u64 v[PG_SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int i = 0; i < PG_SCAN_ITEMS; ++i) {
            v[i] = k0 + i < count ? load(k0 + i) : 0ull;
            sum += v[i];
        }
        pg_u64 inc = sum;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const pg_u64 o = __shfl_up(inc, off, 64);
            if (lane >= off) inc += o;
        }
        __syncthreads();                                           // sm is free (previous tile)
        if (lane == 63) sm[wave] = inc;
        __syncthreads();
        if (threadIdx.x == 0) {
            pg_u64 r = 0;
            for (int i = 0; i < PG_SCAN_THREADS / 64; ++i) { const pg_u64 t = sm[i]; sm[i] = r; r += t; }
            sm[16] = r;
        }
        __syncthreads();
        pg_u64 ex = run + sm[wave] + inc - sum;
#pragma unroll
        for (int i = 0; i < PG_SCAN_ITEMS; ++i) {
            if (k0 + i < count) store(k0 + i, ex);
            ex += v[i];
        }
        run += sm[16];
    }
    return run;
}

// 2. grid n: segment counts -> first compact index per segment, edges per mask
__global__ __launch_bounds__(PG_SCAN_THREADS) void pg_seg_scan_kernel(PgScratch sc) {
    __shared__ pg_u64 sm[17];
    const int m = blockIdx.x;
    uint32_t* so = sc.segoff + (size_t)m * sc.ns;
    const pg_u64 total = pg_block_scan(sc.ns, [&](size_t k) { return (pg_u64)so[k]; }, [&](size_t k, pg_u64 e) { so[k] = (uint32_t)e; }, sm);
    if (threadIdx.x == 0) sc.totals[4 * m] = (int32_t)total;      // < 4 h w < 2^32; above 2^31 - 1 it reads as negative: over any cap
}

// edges of mask m, or -1 when the mask is over the cap (or its count does not fit int32) and is not traced
__device__ __forceinline__ int pg_edges(const PgScratch& sc, int m, int max_edges) {
    const int ne = sc.totals[4 * m];
    return (ne < 0 || ne > max_edges || (size_t)ne > sc.ecap) ? -1 : ne;
}

__device__ __forceinline__ bool pg_set(const uint8_t* __restrict__ mk, int h, int w, int x, int y) {
    return x >= 0 && y >= 0 && x < w && y < h && mk[(size_t)y * w + x] != 0;
}

// compact index of edge d of the set pixel (x, y), which has that edge
__device__ __forceinline__ int pg_index(const uint2* __restrict__ sb, const uint32_t* __restrict__ so, int sr, int x, int y, int d) {
    const size_t s = (size_t)y * sr + (x >> 4);
    const uint2 q = sb[s];
    const int i = x & 15;
    const uint32_t below = (1u << i) - 1u;
    const uint32_t lo = below | (below << 16);
    int idx = (int)so[s] + __popc(q.x & lo) + __popc(q.y & lo);
    const uint32_t here = ((q.x >> i) & 1u) | (((q.x >> (16 + i)) & 1u) << 1) | (((q.y >> i) & 1u) << 2) | (((q.y >> (16 + i)) & 1u) << 3);
    return idx + __popc(here & ((1u << d) - 1u));
}

// 3. grid (ceil(NS / 256), n): thread = segment
__global__ __launch_bounds__(256) void pg_link_kernel(const uint8_t* __restrict__ masks, int h, int w, int sr, int max_edges,
                                                      PgScratch sc) {
    const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= sc.ns) return;
    const int m = blockIdx.y;
    const int ne = pg_edges(sc, m, max_edges);
    if (ne <= 0) return;
    const uint2* __restrict__ sb = sc.segbits + (size_t)m * sc.ns;
    const uint32_t* __restrict__ so = sc.segoff + (size_t)m * sc.ns;
    const uint2 q = sb[s];
    uint32_t any = (q.x | (q.x >> 16) | q.y | (q.y >> 16)) & 0xffffu;
    if (!any) return;
    const uint8_t* __restrict__ mk = masks + (size_t)m * h * w;
    const int y = (int)(s / sr), xb = (int)(s % sr) * 16;
    int idx = (int)so[s];
    const size_t eb = (size_t)m * sc.ecap;
    while (any) {
        const int i = __ffs((int)any) - 1;
        any &= any - 1;
        const int x = xb + i;
        const uint32_t here = ((q.x >> i) & 1u) | (((q.x >> (16 + i)) & 1u) << 1) | (((q.y >> i) & 1u) << 2) | (((q.y >> (16 + i)) & 1u) << 3);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
            if (!((here >> d) & 1u)) continue;
            const int dx = d == 0 ? 1 : (d == 2 ? -1 : 0), dy = d == 1 ? 1 : (d == 3 ? -1 : 0);
            const int dl = (d + 3) & 3;                            // the left of the heading
            const int lx = dl == 0 ? 1 : (dl == 2 ? -1 : 0), ly = dl == 1 ? 1 : (dl == 3 ? -1 : 0);
            int sx, sy, sd;
            if (pg_set(mk, h, w, x + dx + lx, y + dy + ly)) { sx = x + dx + lx; sy = y + dy + ly; sd = dl; }
            else if (pg_set(mk, h, w, x + dx, y + dy)) { sx = x + dx; sy = y + dy; sd = d; }
            else { sx = x; sy = y; sd = (d + 1) & 3; }
            const int sidx = pg_index(sb, so, sr, sx, sy, sd);
            // the predecessor runs straight into this edge iff the pixel behind is set and the one behind on the left is not
            const bool straight = pg_set(mk, h, w, x - dx, y - dy) && !pg_set(mk, h, w, x - dx + lx, y - dy + ly);
            if (idx < ne) {
                sc.eid[eb + idx] = 4u * (uint32_t)((size_t)y * w + x) + (uint32_t)d;
                sc.succ[eb + idx] = sidx;
                sc.corner[eb + idx] = straight ? 0 : 1;
                sc.stA[eb + idx] = make_int4(sidx, idx, 0, 0);
            }
            ++idx;
        }
    }
}

// 4. grid (ceil(ecap / 256), n): one round of pointer doubling, src -> dst
__global__ __launch_bounds__(256) void pg_double_kernel(const int4* __restrict__ src, int4* __restrict__ dst, int k, int max_edges,
                                                        PgScratch sc) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int m = blockIdx.y;
    const int ne = pg_edges(sc, m, max_edges);
    if (ne <= 0 || i >= (size_t)ne) return;
    const size_t eb = (size_t)m * sc.ecap;
    int4 a = src[eb + i];
    const int j = (unsigned)a.x < (unsigned)ne ? a.x : (int)i;
    const int4 b = src[eb + j];
    if (b.y < a.y) { a.y = b.y; a.z = b.z + (int)(1u << k); }
    a.x = b.x;
    dst[eb + i] = a;
}

// 5. grid (ceil(ecap / 256), n): leader, rank, and the scan input of the rings
__global__ __launch_bounds__(256) void pg_rank_kernel(const int4* __restrict__ fin, int max_edges, PgScratch sc) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int m = blockIdx.y;
    const int ne = pg_edges(sc, m, max_edges);
    if (ne <= 0 || i >= (size_t)ne) return;
    const size_t eb = (size_t)m * sc.ecap, lb = (size_t)m * (sc.ecap + 1);
    const int4 a = fin[eb + i];
    const int ld = (unsigned)a.y < (unsigned)ne ? a.y : (int)i;
    const int sl = sc.succ[eb + ld];
    const int L = fin[eb + ((unsigned)sl < (unsigned)ne ? sl : ld)].z + 1;
    sc.lead[eb + i] = ld;
    sc.rank[eb + i] = (L - a.z) % L;
    sc.lr[lb + i] = ld == (int)i ? ((1ull << 32) | (pg_u64)(uint32_t)L) : 0ull;
}

// 6. grid n
__global__ __launch_bounds__(PG_SCAN_THREADS) void pg_ring_scan_kernel(int max_edges, PgScratch sc) {
    __shared__ pg_u64 sm[17];
    const int m = blockIdx.x;
    const int ne = pg_edges(sc, m, max_edges);
    if (ne < 0) return;
    pg_u64* lr = sc.lr + (size_t)m * (sc.ecap + 1);
    const pg_u64 total = pg_block_scan((size_t)ne, [&](size_t k) { return lr[k]; }, [&](size_t k, pg_u64 e) { lr[k] = e; }, sm);
    if (threadIdx.x == 0) sc.totals[4 * m + 1] = (int32_t)(total >> 32);
}

// 7. grid (ceil(ecap / 256), n): thread = edge
__global__ __launch_bounds__(256) void pg_scatter_kernel(int w, int max_edges, PgScratch sc) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int m = blockIdx.y;
    const int ne = pg_edges(sc, m, max_edges);
    if (ne <= 0 || i >= (size_t)ne) return;
    const size_t eb = (size_t)m * sc.ecap, lb = (size_t)m * (sc.ecap + 1);
    const int ld = sc.lead[eb + i];
    const uint32_t pos = (uint32_t)sc.lr[lb + ld] + (uint32_t)sc.rank[eb + i];
    if (pos >= (uint32_t)ne) return;
    const uint32_t id = sc.eid[eb + i];
    const int d = (int)(id & 3u), p = (int)(id >> 2), x = p % w, y = p / w;
    // start vertex and the shoelace term xs ye - xe ys of the unit edge: E -y, S +x, W +y, N -x (at the edge's line)
    const int vx = x + (d == 1 || d == 2), vy = y + (d >= 2);
    const int term = d == 0 ? -vy : d == 1 ? vx : d == 2 ? vy : -vx;
    const int c = sc.corner[eb + i];
    sc.pvert[eb + pos] = c ? ((vy << 16) | vx) : -1;
    sc.cs[lb + pos] = ((pg_u64)(uint32_t)term << 32) | (pg_u64)c;
}

// 8. grid n
__global__ __launch_bounds__(PG_SCAN_THREADS) void pg_corner_scan_kernel(int max_edges, PgScratch sc) {
    __shared__ pg_u64 sm[17];
    const int m = blockIdx.x;
    const int ne = pg_edges(sc, m, max_edges);
    if (ne < 0) return;
    pg_u64* cs = sc.cs + (size_t)m * (sc.ecap + 1);
    const pg_u64 total = pg_block_scan((size_t)ne, [&](size_t k) { return cs[k]; }, [&](size_t k, pg_u64 e) { cs[k] = e; }, sm);
    if (threadIdx.x == 0) {
        cs[ne] = total;
        sc.totals[4 * m + 2] = (int32_t)(uint32_t)total;
    }
}

// 9. one thread: the masks of the chunk in order behind the cursor
__global__ void pg_place_kernel(int n, int max_edges, long long vcap, long long rcap, long long* __restrict__ cursor,
                                long long* __restrict__ table, PgScratch sc) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long vf = cursor[0], rf = cursor[1];
    for (int j = 0; j < n; ++j) {
        long long* t = table + (size_t)j * 5;
        const int raw = sc.totals[4 * j];
        t[4] = (long long)(uint32_t)raw;
        sc.placed[2 * j] = sc.placed[2 * j + 1] = -1;
        if (pg_edges(sc, j, max_edges) < 0) { t[0] = -1; t[1] = -1; t[2] = -1; t[3] = -1; continue; }
        const long long nr = sc.totals[4 * j + 1], nv = sc.totals[4 * j + 2];
        if (vf >= 0 && rf >= 0 && vf + nv <= vcap && rf + nr <= rcap) {
            t[0] = rf; t[1] = nr; t[2] = vf; t[3] = nv;
            sc.placed[2 * j] = rf; sc.placed[2 * j + 1] = vf;
            rf += nr; vf += nv;
        } else {
            t[0] = -1; t[1] = -1 - nr; t[2] = -1; t[3] = -1 - nv;
        }
    }
    cursor[0] = vf; cursor[1] = rf;
}

// 10. grid (ceil(ecap / 256), n): thread i = position i (its vertex) and edge i (its ring record when it is a leader)
__global__ __launch_bounds__(256) void pg_emit_kernel(int x0, int y0, int max_edges, int32_t* __restrict__ vertices,
                                                      int32_t* __restrict__ rings, PgScratch sc) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int m = blockIdx.y;
    const int ne = pg_edges(sc, m, max_edges);
    if (ne <= 0 || i >= (size_t)ne) return;
    const long long rf = sc.placed[2 * m], vf = sc.placed[2 * m + 1];
    if (rf < 0 || vf < 0) return;
    const size_t eb = (size_t)m * sc.ecap, lb = (size_t)m * (sc.ecap + 1);
    const int pv = sc.pvert[eb + i];
    if (pv >= 0) {
        int32_t* o = vertices + ((size_t)vf + (uint32_t)sc.cs[lb + i]) * 2;
        o[0] = x0 + (pv & 0xffff);
        o[1] = y0 + (pv >> 16);
    }
    if (sc.lead[eb + i] == (int)i) {
        const pg_u64 r = sc.lr[lb + i];
        // lr is an exclusive scan, so the next entry minus this one is what pg_rank_kernel fed it here: 1 << 32 | L.  A leader is
        // never a mask's last edge (a ring has at least 4 edges and the leader is its smallest index), so i + 1 < ne.
        const uint32_t base = (uint32_t)r, len = (uint32_t)(sc.lr[lb + i + 1] - r);
        const pg_u64 c0 = sc.cs[lb + base], c1 = sc.cs[lb + base + len];
        int32_t* o = rings + ((size_t)rf + (uint32_t)(r >> 32)) * 4;
        o[0] = (int32_t)(uint32_t)c0;
        o[1] = (int32_t)((uint32_t)c1 - (uint32_t)c0);
        o[2] = (int32_t)((uint32_t)(c1 >> 32) - (uint32_t)(c0 >> 32));
        o[3] = (int32_t)(sc.eid[eb + i] >> 2);
    }
}

}  // namespace

bool mask_polygons_shape_ok(int h, int w, int x0, int y0) {
    return mask_boxes_shape_ok(h, w, x0, y0) && (size_t)h * w < (1ull << 30);
}

// edge capacity per mask: a mask has fewer than 4 h w edges, whatever the cap
static inline size_t pg_ecap(int h, int w, int max_edges) {
    const size_t all = 4 * (size_t)h * w;
    return (size_t)max_edges < all ? (size_t)max_edges : all;
}
static inline size_t pg_al(size_t b) { return (b + 255) & ~(size_t)255; }

long long mask_polygons_edge_stride(int h, int w, int max_edges) { return (long long)pg_ecap(h, w, max_edges); }

size_t mask_polygons_scratch_bytes(int n, int h, int w, int max_edges) {
    const size_t ns = (size_t)h * ((w + 15) / 16), e = pg_ecap(h, w, max_edges), N = (size_t)n;
    return pg_al(N * ns * 8) + pg_al(N * ns * 4) + 5 * pg_al(N * e * 4) + pg_al(N * e) + 2 * pg_al(N * e * 16) + 2 * pg_al(N * (e + 1) * 8) +
           pg_al(N * 16) + pg_al(N * 16);
}

static PgScratch pg_carve(void* scratch, int n, int h, int w, int max_edges) {
    const size_t ns = (size_t)h * ((w + 15) / 16), e = pg_ecap(h, w, max_edges), N = (size_t)n;
    unsigned char* p = reinterpret_cast<unsigned char*>(scratch);
    PgScratch sc;
#define PG_TAKE(field_, type_, bytes_) sc.field_ = reinterpret_cast<type_*>(p); p += pg_al(bytes_);
    PG_TAKE(stA, int4, N * e * 16)
    PG_TAKE(stB, int4, N * e * 16)
    PG_TAKE(segbits, uint2, N * ns * 8)
    PG_TAKE(lr, pg_u64, N * (e + 1) * 8)
    PG_TAKE(cs, pg_u64, N * (e + 1) * 8)
    PG_TAKE(placed, long long, N * 16)
    PG_TAKE(segoff, uint32_t, N * ns * 4)
    PG_TAKE(eid, uint32_t, N * e * 4)
    PG_TAKE(succ, int32_t, N * e * 4)
    PG_TAKE(lead, int32_t, N * e * 4)
    PG_TAKE(rank, int32_t, N * e * 4)
    PG_TAKE(pvert, int32_t, N * e * 4)
    PG_TAKE(totals, int32_t, N * 16)
    PG_TAKE(corner, uint8_t, N * e)
#undef PG_TAKE
    sc.ns = ns;
    sc.ecap = e;
    return sc;
}

// stages 1 - 3 (upto = 1), - 5 (2), all (3)
static hipError_t pg_run(const uint8_t* masks, int n, int h, int w, int x0, int y0, int max_edges, void* scratch, int upto,
                         int32_t* vertices, long long vcap, int32_t* rings, long long rcap, long long* cursor, long long* table,
                         hipStream_t s, PgScratch* sc_out) {
    if (!masks || !scratch || n < 1 || n > 65535 || max_edges < 4 || !mask_polygons_shape_ok(h, w, x0, y0)) return hipErrorInvalidValue;
    const PgScratch sc = pg_carve(scratch, n, h, w, max_edges);
    if (sc_out) *sc_out = sc;
    const int sr = (w + 15) / 16;
    const size_t sblocks = (sc.ns + 255) / 256, eblocks = (sc.ecap + 255) / 256;
    if (sblocks > 0x7fffffffull || eblocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 sgrid((unsigned)sblocks, n), egrid((unsigned)eblocks, n);
    if ((w & 15) == 0 && (((uintptr_t)masks) & 15) == 0) pg_seg_bits_kernel<true><<<sgrid, 256, 0, s>>>(masks, h, w, sr, sc);
    else pg_seg_bits_kernel<false><<<sgrid, 256, 0, s>>>(masks, h, w, sr, sc);
    pg_seg_scan_kernel<<<n, PG_SCAN_THREADS, 0, s>>>(sc);
    pg_link_kernel<<<sgrid, 256, 0, s>>>(masks, h, w, sr, max_edges, sc);
    if (upto < 2) return hipGetLastError();
    int rounds = 0;
    while (((size_t)1 << rounds) < sc.ecap) ++rounds;              // 2^rounds >= the longest ring that is traced
    const int4* fin = sc.stA;
    for (int k = 0; k < rounds; ++k) {
        const int4* src = (k & 1) ? sc.stB : sc.stA;
        int4* dst = (k & 1) ? sc.stA : sc.stB;
        pg_double_kernel<<<egrid, 256, 0, s>>>(src, dst, k, max_edges, sc);
        fin = dst;
    }
    pg_rank_kernel<<<egrid, 256, 0, s>>>(fin, max_edges, sc);
    if (upto < 3) return hipGetLastError();
    pg_ring_scan_kernel<<<n, PG_SCAN_THREADS, 0, s>>>(max_edges, sc);
    pg_scatter_kernel<<<egrid, 256, 0, s>>>(w, max_edges, sc);
    pg_corner_scan_kernel<<<n, PG_SCAN_THREADS, 0, s>>>(max_edges, sc);
    pg_place_kernel<<<1, 64, 0, s>>>(n, max_edges, vcap, rcap, cursor, table, sc);
    pg_emit_kernel<<<egrid, 256, 0, s>>>(x0, y0, max_edges, vertices, rings, sc);
    return hipGetLastError();
}

hipError_t launch_mask_polygons(const uint8_t* masks, int n, int h, int w, int x0, int y0, int max_edges, void* scratch,
                                int32_t* vertices, long long vertex_capacity, int32_t* rings, long long ring_capacity,
                                long long* cursor, long long* table, hipStream_t s) {
    if (!vertices || !rings || !cursor || !table || vertex_capacity < 0 || ring_capacity < 0) return hipErrorInvalidValue;
    return pg_run(masks, n, h, w, x0, y0, max_edges, scratch, 3, vertices, vertex_capacity, rings, ring_capacity, cursor, table, s, nullptr);
}

hipError_t launch_polygon_edges(const uint8_t* masks, int n, int h, int w, int max_edges, void* scratch, uint32_t* ids_out,
                                int32_t* succ_out, uint8_t* corner_out, int32_t* counts_out, hipStream_t s) {
    if (!ids_out || !succ_out || !corner_out || !counts_out) return hipErrorInvalidValue;
    PgScratch sc;
    HIP_CHECK_RET(pg_run(masks, n, h, w, 0, 0, max_edges, scratch, 1, nullptr, 0, nullptr, 0, nullptr, nullptr, s, &sc));
    const size_t ne = (size_t)n * sc.ecap;
    HIP_CHECK_RET(hipMemcpyAsync(ids_out, sc.eid, ne * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(succ_out, sc.succ, ne * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(corner_out, sc.corner, ne, hipMemcpyDeviceToDevice, s));
    return hipMemcpy2DAsync(counts_out, 4, sc.totals, 16, 4, n, hipMemcpyDeviceToDevice, s);
}

hipError_t launch_polygon_ranks(const uint8_t* masks, int n, int h, int w, int max_edges, void* scratch, int32_t* leader_out,
                                int32_t* rank_out, int32_t* counts_out, hipStream_t s) {
    if (!leader_out || !rank_out || !counts_out) return hipErrorInvalidValue;
    PgScratch sc;
    HIP_CHECK_RET(pg_run(masks, n, h, w, 0, 0, max_edges, scratch, 2, nullptr, 0, nullptr, 0, nullptr, nullptr, s, &sc));
    const size_t ne = (size_t)n * sc.ecap;
    HIP_CHECK_RET(hipMemcpyAsync(leader_out, sc.lead, ne * 4, hipMemcpyDeviceToDevice, s));
    HIP_CHECK_RET(hipMemcpyAsync(rank_out, sc.rank, ne * 4, hipMemcpyDeviceToDevice, s));
    return hipMemcpy2DAsync(counts_out, 4, sc.totals, 16, 4, n, hipMemcpyDeviceToDevice, s);
}
