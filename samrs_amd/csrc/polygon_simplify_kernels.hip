// polygon_simplify_kernels.hip -- the rings that polygon_kernels.hip traced, simplified in place on the device (gfx950): Douglas-Peucker
// on every closed ring, distances to the chord SEGMENT, 64-bit integers only.
//
// Definition: include/samrs_hip.h samrs_simplify_polygons states the rule (anchors A, B, C; chain (i, j); N, D; the threshold
// N > floor(eps_q^2 D / 256)); tests/polygon_simplify_ref.py restates it as a plain recursion over Python ints and
// tests/test_polygon_simplify_gpu.py asks for exact equality of vertices, ring records, table and cursor.
//
// Rounds, not recursion.  The state of a ring of k vertices: keep[m] (0 undecided, 1 kept, 2 dropped, 3 kept in the round just run),
// lft[m] = the kept vertex that starts m's chain, and per kept vertex i ("the slot of chain (i, j)"): rgt[i] = j (k stands for index
// 0 again), best[i] = the greatest N of the chain, widx[i] = the smallest index that reaches it.  One round, every undecided vertex:
//   1. N(m) against its chain's segment, max into best[lft[m]] (one atomic per wave where a wave's vertices share the chain);
//   2. the vertices with N == best: min of m into widx[lft[m]] -- the key (N descending, index ascending) in two steps, since N needs 54
//      bits and the index 32;
//   3. best <= floor(eps_q^2 D / 256): dropped.  Else the winner becomes kept and takes over the chain's right end (rgt[w] = j), the
//      vertices behind it move to the new chain (lft[m] = w); rgt[i] = w is written at the start of the next round, when no vertex
//      reads rgt[i] any more.
// The loop over rounds runs inside the kernel until a round keeps nothing (__syncthreads_or; at most k rounds: every round keeps a
// vertex or is the last); max and min are order-free, so the result is bitwise reproducible.  Nothing is read back by the host.
// The stages, on the caller's stream, every cross-workgroup dependence a kernel boundary:
//   1. ps_rows_kernel    one workgroup: which rows are placed, exclusive scan of their ring counts = the ring ordinals, v0;
//   2. ps_list_kernel    thread = ring ordinal: its row (binary search), absolute first vertex, k, absolute ring index;
//   3. ps_lds_kernel     <64 threads>   rings of k <= 64: one wave each, state in LDS, barriers are free (the many tiny rings of
//                                       speckle: the workgroups walk the list, no launch slot per ring);
//                        <256 threads>  rings of 65 <= k <= 2048: one workgroup each, vertices and state in 58 KiB of LDS;
//      ps_big_kernel     <1024 threads> longer rings: the same rounds with the state in global scratch (best aliases the ring's own
//                                       part of the staging copy, which is written when the rounds are over);
//      each then ranks its kept vertices (ballot + popcount scan), writes them to the staging copy at the ring's OLD first vertex,
//      the keep flags and the ring's kept count;
//   4. ps_scan_kernel    one workgroup: exclusive scan of the kept counts over the ordinals = every ring's new first vertex; cursor[0];
//   5. ps_finish_kernel  staging copy -> vertices at the new place (the source is never the buffer written: in place is safe), ring
//                        records' first vertex and count, rows' first vertex and count.
// A table or ring record that does not describe what samrs_mask_polygons writes (negative or out-of-capacity fields) makes its row
// pass through or its ring count as empty; more rings than ring_capacity in all: the call changes nothing.  No store leaves the
// capacities.  No inline assembly, no scalar-memory instructions: vector stores and plain C++.
#include "common.h"
#include "kernels.h"

namespace {

typedef unsigned long long ps_u64;
constexpr int PS_WAVE_MAX = 64;        // rings up to here: one wave
constexpr int PS_LDS_MAX = 2048;       // rings up to here: one 256-thread workgroup, state in LDS
constexpr int PS_BIG_THREADS = 1024;
constexpr int PS_SCAN_THREADS = 1024;

struct PsScratch {
    uint8_t* keep;         // [vcap] absolute vertex index: 1 kept (the rounds of the long rings also hold 0, 2, 3 here)
    int32_t* lft;          // [vcap] long rings: the state of the rounds
    int32_t* rgt;          // [vcap]
    uint32_t* widx;        // [vcap]
    ps_u64* best;          // [vcap] = stage
    int2* stage;           // [vcap] a ring's kept vertices in order, from the ring's old first vertex on
    long long* rstart;     // [rcap] by ring ordinal: absolute first vertex
    long long* rabs;       // [rcap] absolute ring index
    int32_t* rk;           // [rcap] vertices
    int32_t* rrow;         // [rcap] row of the table
    int32_t* kept;         // [rcap] kept vertices
    long long* pre;        // [rcap + 1] exclusive scan of kept
    long long* rowbase;    // [n + 1] exclusive scan of the placed rows' ring counts: a row's first ring ordinal
    long long* totals;     // [4] rings in all (-1: more than rcap, nothing is done), v0, placed rows, kept vertices in all
    long long vcap, rcap;
};

// a row that samrs_mask_polygons placed and whose fields stay inside the capacities
__device__ __forceinline__ bool ps_row_ok(const long long* __restrict__ t, long long vcap, long long rcap) {
    return t[0] >= 0 && t[1] >= 0 && t[2] >= 0 && t[3] >= 0 && t[1] <= rcap && t[0] <= rcap - t[1] && t[3] <= vcap && t[2] <= vcap - t[3];
}

// exclusive scan by the whole block (PS_SCAN_THREADS threads) of load(i), i < count; store(i, prefix); returns the total.  sm: LDS [17]
template <class Load, class Store>
__device__ __forceinline__ long long ps_block_scan(long long count, Load load, Store store, long long* sm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long run = 0;
    for (long long t0 = 0; t0 < count; t0 += PS_SCAN_THREADS) {
        const long long i = t0 + threadIdx.x;
        const long long v = i < count ? load(i) : 0ll;
        long long inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const long long o = __shfl_up(inc, off, 64);
            if (lane >= off) inc += o;
        }
        __syncthreads();                                           // sm is free (previous tile)
        if (lane == 63) sm[wave] = inc;
        __syncthreads();
        if (threadIdx.x == 0) {
            long long r = 0;
            for (int k = 0; k < PS_SCAN_THREADS / 64; ++k) { const long long t = sm[k]; sm[k] = r; r += t; }
            sm[16] = r;
        }
        __syncthreads();
        if (i < count) store(i, run + sm[wave] + inc - v);
        run += sm[16];
    }
    return run;
}

// 1. one workgroup
__global__ __launch_bounds__(PS_SCAN_THREADS) void ps_rows_kernel(const long long* __restrict__ table, int n, PsScratch sc) {
    __shared__ long long sm[17];
    __shared__ int first, placed;
    if (threadIdx.x == 0) { first = n; placed = 0; }
    __syncthreads();
    int mine = 0, lo = n;
    for (int j = threadIdx.x; j < n; j += PS_SCAN_THREADS)
        if (ps_row_ok(table + (size_t)j * 5, sc.vcap, sc.rcap)) { ++mine; lo = j < lo ? j : lo; }
    if (mine) { atomicAdd(&placed, mine); atomicMin(&first, lo); }
    const long long total = ps_block_scan(
        n, [&](long long j) { const long long* t = table + (size_t)j * 5; return ps_row_ok(t, sc.vcap, sc.rcap) ? t[1] : 0ll; },
        [&](long long j, long long e) { sc.rowbase[j] = e; }, sm);
    __syncthreads();
    if (threadIdx.x == 0) {
        sc.rowbase[n] = total;
        sc.totals[0] = total > sc.rcap ? -1 : total;
        sc.totals[1] = first < n ? table[(size_t)first * 5 + 2] : 0;
        sc.totals[2] = placed;
        sc.totals[3] = 0;
    }
}

// 2. thread = ring ordinal (grid-stride)
__global__ __launch_bounds__(256) void ps_list_kernel(const int32_t* __restrict__ rings, const long long* __restrict__ table, int n,
                                                      PsScratch sc) {
    const long long R = sc.totals[0];
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < R; o += (long long)gridDim.x * 256) {
        int lo = 0, hi = n;                                        // the last row j with rowbase[j] <= o: rows without rings are passed
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (sc.rowbase[mid] <= o) lo = mid; else hi = mid;
        }
        const long long* t = table + (size_t)lo * 5;
        const long long r = t[0] + (o - sc.rowbase[lo]);
        const int32_t* rec = rings + (size_t)r * 4;
        long long f = rec[0], k = rec[1];
        if (f < 0 || k < 0 || k > t[3] || f > t[3] - k) { f = 0; k = 0; }
        sc.rstart[o] = t[2] + f;
        sc.rabs[o] = r;
        sc.rk[o] = (int32_t)k;
        sc.rrow[o] = lo;
        sc.kept[o] = 0;
    }
}

// the views of one ring's vertices and state: LDS or global
struct PsRing {
    const int2* v;
    uint8_t* keep;
    int32_t* lft;
    int32_t* rgt;
    uint32_t* widx;
    ps_u64* best;
};

// numerator N and denominator D of the squared distance of p to the segment a b (samrs_hip.h)
__device__ __forceinline__ void ps_dist(const int2 a, const int2 b, const int2 p, long long& N, long long& D) {
    const long long bx = (long long)b.x - a.x, by = (long long)b.y - a.y, px = (long long)p.x - a.x, py = (long long)p.y - a.y;
    const long long L = bx * bx + by * by, pa = px * px + py * py;
    if (L == 0) { N = pa; D = 1; return; }
    D = L;
    const long long t = px * bx + py * by;
    if (t <= 0) N = pa * L;
    else if (t >= L) {
        const long long qx = (long long)p.x - b.x, qy = (long long)p.y - b.y;
        N = (qx * qx + qy * qy) * L;
    } else {
        const long long c = bx * py - by * px;
        N = c * c;
    }
}

__device__ __forceinline__ ps_u64 ps_wave_max(ps_u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const ps_u64 o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}
// greatest value, smallest index: value in the high word (at most 2^27 within the limits), ~index in the low one
__device__ __forceinline__ ps_u64 ps_key(long long val, int m) {
    const ps_u64 a = (ps_u64)(val < 0 ? -val : val);
    return ((a > 0xffffffffull ? 0xffffffffull : a) << 32) | (ps_u64)(0xffffffffu - (uint32_t)m);
}

// the rule on one ring by the whole workgroup of T threads; k >= 1.  sm: LDS ps_u64 [2].  Ends with keep[m] & 1 = kept, behind a barrier.
template <int T>
__device__ __forceinline__ void ps_rounds(const PsRing g, const int k, const long long eps2, ps_u64* sm) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (k <= 3) {                                                  // no lattice ring; nothing to drop
        for (int m = tid; m < k; m += T) g.keep[m] = 1;
        __syncthreads();
        return;
    }
    if (tid == 0) { sm[0] = 0; sm[1] = 0; }
    __syncthreads();
    const int2 vA = g.v[0];
    // anchor B: the farthest from v[0]
    {
        ps_u64 key = 0;
        for (int m = tid; m < k; m += T) {
            const int2 p = g.v[m];
            const long long dx = (long long)p.x - vA.x, dy = (long long)p.y - vA.y;
            const ps_u64 c = ps_key(dx * dx + dy * dy, m);
            key = c > key ? c : key;
        }
        key = ps_wave_max(key);
        if (lane == 0) atomicMax(&sm[0], key);
    }
    __syncthreads();
    const int iB = (int)(0xffffffffu - (uint32_t)sm[0]);
    const int2 vB = g.v[iB];
    // anchor C: the greatest |cross| against A B
    {
        const long long bx = (long long)vB.x - vA.x, by = (long long)vB.y - vA.y;
        ps_u64 key = 0;
        for (int m = tid; m < k; m += T) {
            const int2 p = g.v[m];
            const long long px = (long long)p.x - vA.x, py = (long long)p.y - vA.y;
            const ps_u64 c = ps_key(bx * py - by * px, m);
            key = c > key ? c : key;
        }
        key = ps_wave_max(key);
        if (lane == 0) atomicMax(&sm[1], key);
    }
    __syncthreads();
    const int iC = (int)(0xffffffffu - (uint32_t)sm[1]);
    const int s1 = iB < iC ? iB : iC, s2 = iB < iC ? iC : iB;      // a degenerate ring repeats an anchor: harmless below
    for (int m = tid; m < k; m += T) {
        if (m == 0 || m == s1 || m == s2) {
            int r = k;
            if (s2 > m) r = s2;
            if (s1 > m) r = s1;
            g.keep[m] = 1;
            g.rgt[m] = r;
        } else {
            g.keep[m] = 0;
            g.lft[m] = s2 <= m ? s2 : (s1 <= m ? s1 : 0);
        }
    }
    __syncthreads();
    for (int round = 0; round < k; ++round) {
        // the winners of the last round join their left neighbour's chain; every kept vertex clears its slot
        for (int m = tid; m < k; m += T) {
            int f = g.keep[m];
            if (f == 3) { g.rgt[g.lft[m]] = m; g.keep[m] = 1; f = 1; }
            if (f == 1) { g.best[m] = 0; g.widx[m] = 0xffffffffu; }
        }
        __syncthreads();
        // 1. the greatest N of every chain
        for (int m0 = 0; m0 < k; m0 += T) {
            const int m = m0 + tid;
            const bool act = m < k && g.keep[m] == 0;
            int i = -1;
            long long N = 0, D = 1;
            if (act) {
                i = g.lft[m];
                const int j = g.rgt[i];
                ps_dist(g.v[i], g.v[j == k ? 0 : j], g.v[m], N, D);
            }
            const ps_u64 mask = __ballot(act);
            if (mask) {
                const int head = __ffsll((long long)mask) - 1;
                const int i0 = __shfl(i, head, 64);
                if (__all(!act || i == i0)) {                      // one chain in the wave: one atomic
                    const ps_u64 best = ps_wave_max((ps_u64)N);
                    if (lane == head) atomicMax(&g.best[i0], best);
                } else if (act) atomicMax(&g.best[i], (ps_u64)N);
            }
        }
        __syncthreads();
        // 2. the smallest index that reaches it
        for (int m = tid; m < k; m += T) {
            if (g.keep[m] != 0) continue;
            const int i = g.lft[m], j = g.rgt[i];
            long long N, D;
            ps_dist(g.v[i], g.v[j == k ? 0 : j], g.v[m], N, D);
            if ((ps_u64)N == g.best[i]) atomicMin(&g.widx[i], (uint32_t)m);
        }
        __syncthreads();
        // 3. keep the winner or drop the chain
        int won = 0;
        for (int m = tid; m < k; m += T) {
            if (g.keep[m] != 0) continue;
            const int i = g.lft[m], j = g.rgt[i];
            const int2 a = g.v[i], b = g.v[j == k ? 0 : j];
            const long long bx = (long long)b.x - a.x, by = (long long)b.y - a.y, L = bx * bx + by * by;
            const long long thr = (eps2 * (L == 0 ? 1 : L)) >> 8;
            const uint32_t w = g.widx[i];
            if (!(g.best[i] > (ps_u64)thr)) g.keep[m] = 2;
            else if ((uint32_t)m == w) { g.keep[m] = 3; g.rgt[m] = j; won = 1; }
            else if ((uint32_t)m > w) g.lft[m] = (int32_t)w;
        }
        if (!__syncthreads_or(won)) break;
    }
}

// the kept vertices of the ring in order -> stage (from the ring's old first vertex on), the flags -> keepg; returns their number.
// smi: LDS int [T / 64].  All threads of the workgroup.
template <int T>
__device__ __forceinline__ int ps_compact(const PsRing g, const int k, uint8_t* keepg, int2* stage, int* smi) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int run = 0;
    for (int m0 = 0; m0 < k; m0 += T) {
        const int m = m0 + tid;
        const int f = m < k ? (g.keep[m] & 1) : 0;
        const int2 p = f ? g.v[m] : make_int2(0, 0);
        const ps_u64 b = __ballot(f);
        const int wr = __popcll(b & ((1ull << lane) - 1ull));
        int before = 0, tot = __popcll(b);
        if (T > 64) {
            __syncthreads();                                       // smi is free (previous tile)
            if (lane == 0) smi[wave] = tot;
            __syncthreads();
            tot = 0;
            for (int q = 0; q < T / 64; ++q) {
                const int c = smi[q];
                before += q < wave ? c : 0;
                tot += c;
            }
        }
        if (m < k) keepg[m] = (uint8_t)f;
        if (f) stage[run + before + wr] = p;
        run += tot;
    }
    return run;
}

// 3. rings of KMIN .. KMAX vertices: workgroup = ring (grid-stride over the ordinals), vertices and state in LDS
template <int T, int KMIN, int KMAX>
__global__ __launch_bounds__(T) void ps_lds_kernel(const int32_t* __restrict__ vertices, int eps_q, PsScratch sc) {
    __shared__ ps_u64 sbest[KMAX];
    __shared__ int2 sv[KMAX];
    __shared__ int32_t slft[KMAX], srgt[KMAX];
    __shared__ uint32_t swidx[KMAX];
    __shared__ uint8_t skeep[KMAX];
    __shared__ ps_u64 sm[2];
    __shared__ int smi[T / 64];
    const long long R = sc.totals[0];
    const long long eps2 = (long long)eps_q * eps_q;
    const PsRing g{sv, skeep, slft, srgt, swidx, sbest};
    for (long long o = blockIdx.x; o < R; o += gridDim.x) {
        const int k = sc.rk[o];
        if (k < KMIN || k > KMAX) continue;
        const long long start = sc.rstart[o];
        const int2* __restrict__ src = reinterpret_cast<const int2*>(vertices) + start;
        for (int m = threadIdx.x; m < k; m += T) sv[m] = src[m];
        __syncthreads();
        ps_rounds<T>(g, k, eps2, sm);
        const int kept = ps_compact<T>(g, k, sc.keep + start, sc.stage + start, smi);
        if (threadIdx.x == 0) sc.kept[o] = kept;
        __syncthreads();                                           // LDS is free for the next ring
    }
}

// 3. longer rings: the same with the state in global scratch
__global__ __launch_bounds__(PS_BIG_THREADS) void ps_big_kernel(const int32_t* __restrict__ vertices, int eps_q, PsScratch sc) {
    __shared__ ps_u64 sm[2];
    __shared__ int smi[PS_BIG_THREADS / 64];
    const long long R = sc.totals[0];
    const long long eps2 = (long long)eps_q * eps_q;
    for (long long o = blockIdx.x; o < R; o += gridDim.x) {
        const int k = sc.rk[o];
        if (k <= PS_LDS_MAX) continue;
        const long long start = sc.rstart[o];
        const PsRing g{reinterpret_cast<const int2*>(vertices) + start, sc.keep + start, sc.lft + start, sc.rgt + start, sc.widx + start,
                       sc.best + start};
        ps_rounds<PS_BIG_THREADS>(g, k, eps2, sm);
        // best is dead: its words become the staging copy.  Entry `rank` is written by the thread that holds vertex m >= rank.
        const int kept = ps_compact<PS_BIG_THREADS>(g, k, sc.keep + start, sc.stage + start, smi);
        if (threadIdx.x == 0) sc.kept[o] = kept;
        __syncthreads();
    }
}

// 4. one workgroup
__global__ __launch_bounds__(PS_SCAN_THREADS) void ps_scan_kernel(long long* __restrict__ cursor, PsScratch sc) {
    __shared__ long long sm[17];
    const long long R = sc.totals[0];
    if (R < 0 || sc.totals[2] == 0) return;
    const long long total = ps_block_scan(
        R, [&](long long o) { return (long long)sc.kept[o]; }, [&](long long o, long long e) { sc.pre[o] = e; }, sm);
    if (threadIdx.x == 0) {
        sc.pre[R] = total;
        sc.totals[3] = total;
        if (cursor) cursor[0] = sc.totals[1] + total;
    }
}

// 5. workgroup = ring (grid-stride): its kept vertices to their new place, its record; thread = row: its first vertex and count
__global__ __launch_bounds__(256) void ps_finish_kernel(int32_t* __restrict__ vertices, int32_t* __restrict__ rings,
                                                        long long* __restrict__ table, int n, PsScratch sc) {
    const long long R = sc.totals[0], v0 = sc.totals[1];
    if (R < 0 || sc.totals[2] == 0) return;
    for (long long o = blockIdx.x; o < R; o += gridDim.x) {
        const int kept = sc.kept[o];
        const long long at = sc.pre[o];
        const int2* __restrict__ src = sc.stage + sc.rstart[o];
        int2* __restrict__ dst = reinterpret_cast<int2*>(vertices) + v0 + at;
        if (v0 + at + kept > sc.vcap) continue;                    // rows that are not behind one another as placed: no store leaves the buffer
        for (int m = threadIdx.x; m < kept; m += 256) dst[m] = src[m];
        if (threadIdx.x == 0) {
            int32_t* rec = rings + (size_t)sc.rabs[o] * 4;
            rec[0] = (int32_t)(at - sc.pre[sc.rowbase[sc.rrow[o]]]);
            rec[1] = kept;
        }
    }
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long long)gridDim.x * 256) {
        long long* t = table + (size_t)j * 5;
        if (!ps_row_ok(t, sc.vcap, sc.rcap)) continue;
        const long long b = sc.pre[sc.rowbase[j]], e = sc.pre[sc.rowbase[j + 1]];
        t[2] = v0 + b;
        t[3] = e - b;
    }
}

// the hook's view: kept counts by absolute ring index
__global__ __launch_bounds__(256) void ps_export_kernel(int32_t* __restrict__ kept_out, PsScratch sc) {
    const long long R = sc.totals[0];
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < R; o += (long long)gridDim.x * 256) kept_out[sc.rabs[o]] = sc.kept[o];
}

inline size_t ps_al(size_t b) { return (b + 255) & ~(size_t)255; }

PsScratch ps_carve(void* scratch, int n, long long vcap, long long rcap) {
    const size_t V = (size_t)vcap, Rr = (size_t)rcap;
    unsigned char* p = reinterpret_cast<unsigned char*>(scratch);
    PsScratch sc;
#define PS_TAKE(field_, type_, bytes_) sc.field_ = reinterpret_cast<type_*>(p); p += ps_al(bytes_);
    PS_TAKE(stage, int2, V * 8)
    PS_TAKE(lft, int32_t, V * 4)
    PS_TAKE(rgt, int32_t, V * 4)
    PS_TAKE(widx, uint32_t, V * 4)
    PS_TAKE(rstart, long long, Rr * 8)
    PS_TAKE(rabs, long long, Rr * 8)
    PS_TAKE(pre, long long, (Rr + 1) * 8)
    PS_TAKE(rowbase, long long, ((size_t)n + 1) * 8)
    PS_TAKE(totals, long long, 32)
    PS_TAKE(rk, int32_t, Rr * 4)
    PS_TAKE(rrow, int32_t, Rr * 4)
    PS_TAKE(kept, int32_t, Rr * 4)
    PS_TAKE(keep, uint8_t, V)
#undef PS_TAKE
    sc.best = reinterpret_cast<ps_u64*>(sc.stage);
    sc.vcap = vcap;
    sc.rcap = rcap;
    return sc;
}

bool ps_args_ok(int n, int eps_q, long long vcap, long long rcap) {
    return n >= 1 && eps_q >= 1 && eps_q <= POLYGON_SIMPLIFY_EPS_MAX && vcap >= 0 && rcap >= 0 && vcap < (1ll << 40) && rcap < (1ll << 40);
}

// stages 1 - 3
hipError_t ps_keep(const int32_t* vertices, const int32_t* rings, const long long* table, int n, int eps_q, const PsScratch& sc,
                   hipStream_t s) {
    ps_rows_kernel<<<1, PS_SCAN_THREADS, 0, s>>>(table, n, sc);
    ps_list_kernel<<<512, 256, 0, s>>>(rings, table, n, sc);
    ps_lds_kernel<64, 1, PS_WAVE_MAX><<<2048, 64, 0, s>>>(vertices, eps_q, sc);
    ps_lds_kernel<256, PS_WAVE_MAX + 1, PS_LDS_MAX><<<512, 256, 0, s>>>(vertices, eps_q, sc);
    ps_big_kernel<<<128, PS_BIG_THREADS, 0, s>>>(vertices, eps_q, sc);
    return hipGetLastError();
}

}  // namespace

size_t polygon_simplify_scratch_bytes(int n, long long vertex_capacity, long long ring_capacity) {
    const size_t V = (size_t)vertex_capacity, R = (size_t)ring_capacity;
    return ps_al(V * 8) + 3 * ps_al(V * 4) + ps_al(V) + 2 * ps_al(R * 8) + ps_al((R + 1) * 8) + 3 * ps_al(R * 4) + ps_al(((size_t)n + 1) * 8) +
           ps_al(32);
}

hipError_t launch_polygon_simplify(int32_t* vertices, int32_t* rings, long long* table, int n, int eps_q, long long vertex_capacity,
                                   long long ring_capacity, void* scratch, long long* cursor, hipStream_t s) {
    if (!vertices || !rings || !table || !cursor || !scratch || !ps_args_ok(n, eps_q, vertex_capacity, ring_capacity))
        return hipErrorInvalidValue;
    const PsScratch sc = ps_carve(scratch, n, vertex_capacity, ring_capacity);
    HIP_CHECK_RET(ps_keep(vertices, rings, table, n, eps_q, sc, s));
    ps_scan_kernel<<<1, PS_SCAN_THREADS, 0, s>>>(cursor, sc);
    ps_finish_kernel<<<1024, 256, 0, s>>>(vertices, rings, table, n, sc);
    return hipGetLastError();
}

hipError_t launch_polygon_simplify_keep(const int32_t* vertices, const int32_t* rings, const long long* table, int n, int eps_q,
                                        long long vertex_capacity, long long ring_capacity, void* scratch, uint8_t* keep_out,
                                        int32_t* kept_out, hipStream_t s) {
    if (!vertices || !rings || !table || !keep_out || !kept_out || !scratch || !ps_args_ok(n, eps_q, vertex_capacity, ring_capacity))
        return hipErrorInvalidValue;
    const PsScratch sc = ps_carve(scratch, n, vertex_capacity, ring_capacity);
    HIP_CHECK_RET(hipMemsetAsync(sc.keep, 0, (size_t)vertex_capacity, s));
    HIP_CHECK_RET(hipMemsetAsync(kept_out, 0xff, (size_t)ring_capacity * 4, s));
    HIP_CHECK_RET(ps_keep(vertices, rings, table, n, eps_q, sc, s));
    ps_export_kernel<<<256, 256, 0, s>>>(kept_out, sc);
    HIP_CHECK_RET(hipGetLastError());
    return hipMemcpyAsync(keep_out, sc.keep, (size_t)vertex_capacity, hipMemcpyDeviceToDevice, s);
}
