// polygon_fill_kernels.hip -- the inverse of polygon_kernels.hip on the device (gfx950): rings with arbitrary integer vertices (traced,
// simplified, or built by a caller) filled even-odd at the pixel centres, 64-bit integers only.
//
// Definition: include/samrs_hip.h samrs_fill_polygons states the rule (which rows an edge acts on, the first column it toggles, the
// tie at a centre on an edge); tests/polygon_fill_ref.py restates it as a per-pixel crossing count over Python ints and
// tests/test_polygon_fill_gpu.py asks for exact equality of every byte and of the three counts.
//
// One kernel, one workgroup of 256 threads per (row of the table, band of PF_BAND_ROWS-or-fewer mask rows); the band's toggle bits live
// in LDS, one bit per pixel, a mask row padded to whole 32-bit words (at most 32 KiB: the band is 64 rows up to w = 4096, 32 beyond):
//   1. the LDS bits are cleared;
//   2. the workgroup walks the row's vertices (thread = vertex, stride 256).  A vertex's successor is the next one, or its ring's first
//      when it is the ring's last: the ring is found by binary search in the row's ring records (ascending first vertex), and kept in
//      registers while the thread's next vertices lie in the same ring.  The edge is clipped to the band; per mask row it crosses, the
//      first toggled column c = ceil(((2 xa - 1) dy + dx (2 r + 1 - 2 ya)) / (2 dy)) (dy > 0 after orienting the edge), clamped to
//      [0, w], is one LDS atomicXor on bit c -- two divisions per edge and band, then quotient and remainder step from mask row to mask
//      row.  XOR is order-free: no global atomics on pixels, no scratch, bitwise reproducible.  The same walk checks what the header
//      asks of a row: every vertex within 2^20 of (x0, y0), and ring records that tile the row's vertex range;
//   3. after a barrier a wave takes a mask row: in-word prefix parity (x ^= x << 1 ... << 16), the carry into a word = the parity of the
//      words before it (their top bits after the prefix, one ballot per 64 words);
//   4. the bits go out as bytes and `ref` comes in, 16 bytes per lane and fully coalesced (lane l owns the half l & 1 of the word of
//      lane l >> 1, fetched by shuffle) where the mask row's first byte and w are multiples of 16, bytewise otherwise; nothing is
//      stored past a mask row.  ref is packed to bits (non-zero = set) and the three counts are popcounts;
//   5. wave shuffle sums -> LDS -> one 64-bit integer atomicAdd per workgroup and non-zero count into counts_out, which the launcher
//      zeroes on the stream first.  A row that is not a set of rings fills as empty and band 0 adds -1 to its first count.
// Cost (tools/polygon_fill_bench.py, profiles/polygon_fill_bench.txt): every band's workgroup repeats the tiling check and the walk over
// all of the row's vertices, 16 times for a 1024-row mask, and that walk, not the h x w pass, is where the time goes (a call takes
// the same time with and without masks_out).  Binning the edges per band in a first kernel would remove the repetition; not built.
// Table and ring fields are untrusted: a row is bounded by its own counts, every read stays inside [first, first + count) of the row's
// vertices and ring records, every store inside [n][h][w] / [n][3].  No inline assembly, no scalar-memory instructions.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int PF_THREADS = 256;
constexpr int PF_WAVES = PF_THREADS / 64;
constexpr int PF_BAND_ROWS = 64;
constexpr int PF_LDS_WORDS = 8192;                 // 32 KiB of toggle bits
constexpr long long PF_REACH = 1ll << 20;          // a vertex farther than this from (x0, y0) in a coordinate: the row is not filled
constexpr long long PF_FIRST_MAX = 1ll << 40;      // table firsts beyond this cannot index a buffer
constexpr int PF_CHUNK = 32768;                    // table rows per launch (grid.y)

__host__ __device__ inline int pf_band_rows(int w) {
    const int wpr = (w + 31) >> 5;
    const int fit = PF_LDS_WORDS / wpr;
    return fit < PF_BAND_ROWS ? fit : PF_BAND_ROWS;
}

// four bits -> four 0 / 1 bytes and back (the partial products never share a bit position: no carries)
__device__ __forceinline__ uint32_t pf_spread4(uint32_t b) { return (b * 0x00204081u) & 0x01010101u; }
__device__ __forceinline__ uint32_t pf_gather4(uint32_t v) {
    const uint32_t nz = ((((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v) >> 7) & 0x01010101u;      // a byte that is not zero
    return ((nz * 0x01020408u) >> 24) & 0xfu;
}
__device__ __forceinline__ uint32_t pf_gather16(const uint4& v) {
    return pf_gather4(v.x) | (pf_gather4(v.y) << 4) | (pf_gather4(v.z) << 8) | (pf_gather4(v.w) << 12);
}

__global__ __launch_bounds__(PF_THREADS) void pf_fill_kernel(const int32_t* __restrict__ vertices, const int32_t* __restrict__ rings,
                                                             const long long* __restrict__ table, int h, int w, int x0, int y0,
                                                             uint8_t* __restrict__ masks_out, const uint8_t* __restrict__ ref,
                                                             unsigned long long* __restrict__ counts_out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t pf_lds[];
    const int wpr = (w + 31) >> 5;
    const int band = pf_band_rows(w);
    uint32_t* bits = pf_lds;                                   // [band][wpr]
    int* red = (int*)(pf_lds + (size_t)band * wpr);            // [PF_WAVES][3]
    const int j = blockIdx.y;
    const int r_lo = blockIdx.x * band;
    const int r_hi = r_lo + band < h ? r_lo + band : h;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    for (int i = threadIdx.x; i < band * wpr; i += PF_THREADS) bits[i] = 0u;

    const long long* t = table + (size_t)j * 5;
    const long long first_ring = t[0], n_rings = t[1], first_vertex = t[2], n_vertices = t[3];
    // a set of rings: counts of a placed row, firsts that can index a buffer; no rings at all is the empty mask
    const bool row_ok = n_rings >= 0 && n_vertices >= 0 && n_rings < (1ll << 30) && n_vertices < (1ll << 30) && first_ring >= 0 &&
                        first_vertex >= 0 && first_ring < PF_FIRST_MAX && first_vertex < PF_FIRST_MAX &&
                        (n_rings > 0 ? n_vertices >= n_rings : n_vertices == 0);
    const int nr = row_ok ? (int)n_rings : 0, nv = row_ok ? (int)n_vertices : 0;
    const int32_t* rec = rings + (size_t)(row_ok ? first_ring : 0) * 4;
    const int32_t* vtx = vertices + (size_t)(row_ok ? first_vertex : 0) * 2;
    int bad = row_ok ? 0 : 1;

    // the ring records tile [0, nv): the first begins at 0, each begins where its predecessor ends, the last ends at nv, none is empty
    for (int q = threadIdx.x; q < nr; q += PF_THREADS) {
        const long long f = rec[(size_t)q * 4], k = rec[(size_t)q * 4 + 1];
        const long long want = q == 0 ? 0ll : (long long)rec[(size_t)(q - 1) * 4] + (long long)rec[(size_t)(q - 1) * 4 + 1];
        if (f != want || k < 1 || f + k > nv || (q == nr - 1 && f + k != nv)) bad = 1;
    }
    bad = __syncthreads_or(bad);                               // also: the LDS bits are cleared
    if (!bad) {
        int rf = 0, rk = 0;                                    // the ring of the thread's last vertex: [rf, rf + rk)
        for (int i = threadIdx.x; i < nv; i += PF_THREADS) {
            if (i >= rf + rk) {                                // the last record with first <= i (the records tile, so it holds i)
                int lo = 0, hi = nr;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (rec[(size_t)mid * 4] <= i) lo = mid; else hi = mid;
                }
                rf = rec[(size_t)lo * 4];
                rk = rec[(size_t)lo * 4 + 1];
            }
            const int nx = i + 1 < rf + rk ? i + 1 : rf;
            const long long xa = (long long)vtx[(size_t)i * 2] - x0, ya = (long long)vtx[(size_t)i * 2 + 1] - y0;
            if (xa > PF_REACH || xa < -PF_REACH || ya > PF_REACH || ya < -PF_REACH) { bad = 1; continue; }
            const long long xb = (long long)vtx[(size_t)nx * 2] - x0, yb = (long long)vtx[(size_t)nx * 2 + 1] - y0;
            if (xb > PF_REACH || xb < -PF_REACH || yb > PF_REACH || yb < -PF_REACH) { bad = 1; continue; }
            if (ya == yb) continue;                            // horizontal edges never count
            long long dx = xb - xa, dy = yb - ya;
            if (dy < 0) { dx = -dx; dy = -dy; }
            const long long e_lo = ya < yb ? ya : yb, e_hi = ya < yb ? yb : ya;
            const int a = e_lo > r_lo ? (int)e_lo : r_lo;      // e_lo <= r < e_hi inside the band
            const int b = e_hi < r_hi ? (int)e_hi : r_hi;
            if (a >= b) continue;
            if (dx == 0) {                                     // every edge of a lattice ring: c = ceil((2 xa - 1) / 2) = xa
                if (xa < w) {
                    const int c = xa < 0 ? 0 : (int)xa;
                    for (int r = a; r < b; ++r) atomicXor(&bits[(size_t)(r - r_lo) * wpr + (c >> 5)], 1u << (c & 31));
                }
                continue;
            }
            // N(r) = (2 xa - 1) dy + dx (2 r + 1 - 2 ya), |N| < 2^45; D = 2 dy; c = ceil(N / D).  Floor quotient and remainder of N(a)
            // and of the step 2 dx, then one add and one compare per mask row
            const long long D = 2 * dy;
            const long long N = (2 * xa - 1) * dy + dx * (2 * (long long)a + 1 - 2 * ya);
            long long q = N / D, rem = N % D;
            if (rem < 0) { rem += D; --q; }
            long long sq = (2 * dx) / D, sr = (2 * dx) % D;
            if (sr < 0) { sr += D; --sq; }
            for (int r = a; r < b; ++r) {
                const long long cc = q + (rem > 0 ? 1 : 0);
                if (cc < w) {
                    const int c = cc < 0 ? 0 : (int)cc;
                    atomicXor(&bits[(size_t)(r - r_lo) * wpr + (c >> 5)], 1u << (c & 31));
                }
                q += sq;
                rem += sr;
                if (rem >= D) { rem -= D; ++q; }
            }
        }
    }
    bad = __syncthreads_or(bad);                               // also: every toggle of the band is in LDS

    // the byte at masks_out[j][r][0] and at ref[j][r][0] is 16-byte aligned for every r: 16-byte accesses
    const size_t mask0 = (size_t)j * h * w;
    const bool vec_out = masks_out && (w & 15) == 0 && (((uintptr_t)masks_out + mask0) & 15) == 0;
    const bool vec_ref = ref && (w & 15) == 0 && (((uintptr_t)ref + mask0) & 15) == 0;
    int c_fill = 0, c_ref = 0, c_both = 0;
    for (int r = r_lo + wave; r < r_hi; r += PF_WAVES) {
        const uint32_t* row = bits + (size_t)(r - r_lo) * wpr;
        const size_t rowbyte = mask0 + (size_t)r * w;
        uint32_t carry = 0;
        for (int k0 = 0; k0 < wpr; k0 += 64) {                 // wave-uniform trip count: the shuffles and the ballot see all lanes
            const int k = k0 + lane;
            uint32_t x = (k < wpr && !bad) ? row[k] : 0u;
            x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16;          // bit i = parity of the toggles at columns <= i
            const unsigned long long tops = __ballot(x >> 31);
            const uint32_t before = (uint32_t)__popcll(tops & ((1ull << lane) - 1ull)) & 1u;
            if ((before ^ carry) & 1u) x = ~x;
            carry ^= (uint32_t)__popcll(tops) & 1u;
            const int left = w - k * 32;                       // columns of this word inside the mask row
            x = left >= 32 ? x : (left <= 0 ? 0u : x & ((1u << left) - 1u));
#pragma unroll
            for (int half = 0; half < 2; ++half) {             // lane l: 16 pixels, the half l & 1 of the word of lane half * 32 + (l >> 1)
                const int src = half * 32 + (lane >> 1);
                const uint32_t xs = (uint32_t)__shfl((int)x, src, 64);
                const int c0 = (k0 + src) * 32 + (lane & 1) * 16;
                if (c0 >= w) continue;
                const uint32_t f16 = (xs >> ((lane & 1) * 16)) & 0xffffu;
                const int nc = w - c0 < 16 ? w - c0 : 16;
                if (masks_out) {
                    uint8_t* o = masks_out + rowbyte + c0;
                    if (vec_out) {
                        uint4 v;
                        v.x = pf_spread4(f16 & 15u); v.y = pf_spread4((f16 >> 4) & 15u);
                        v.z = pf_spread4((f16 >> 8) & 15u); v.w = pf_spread4(f16 >> 12);
                        *reinterpret_cast<uint4*>(o) = v;
                    } else {
                        for (int c = 0; c < nc; ++c) o[c] = (uint8_t)((f16 >> c) & 1u);
                    }
                }
                uint32_t g16 = 0u;
                if (ref) {
                    const uint8_t* g = ref + rowbyte + c0;
                    if (vec_ref) {
                        g16 = pf_gather16(*reinterpret_cast<const uint4*>(g));
                    } else {
                        for (int c = 0; c < nc; ++c) g16 |= (g[c] != 0 ? 1u : 0u) << c;
                    }
                }
                c_fill += __popc(f16);
                c_ref += __popc(g16);
                c_both += __popc(f16 & g16);
            }
        }
    }
    if (!counts_out) return;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c_fill += __shfl_down(c_fill, off, 64);
        c_ref += __shfl_down(c_ref, off, 64);
        c_both += __shfl_down(c_both, off, 64);
    }
    if (lane == 0) { red[wave * 3] = c_fill; red[wave * 3 + 1] = c_ref; red[wave * 3 + 2] = c_both; }
    __syncthreads();
    if (threadIdx.x < 3) {
        long long s = 0;
        for (int wv = 0; wv < PF_WAVES; ++wv) s += red[wv * 3 + threadIdx.x];
        if (threadIdx.x == 0 && bad && blockIdx.x == 0) s = -1;                        // a bad row toggles nothing: its fill count is 0
        if (s != 0) atomicAdd(&counts_out[(size_t)j * 3 + threadIdx.x], (unsigned long long)s);
    }
}

}  // namespace

hipError_t launch_fill_polygons(const int32_t* vertices, const int32_t* rings, const long long* table, int n, int h, int w, int x0,
                                int y0, uint8_t* masks_out, const uint8_t* ref, long long* counts_out, hipStream_t s) {
    if (n < 1) return hipSuccess;
    if (counts_out) {
        const hipError_t r = hipMemsetAsync(counts_out, 0, (size_t)n * 3 * sizeof(long long), s);
        if (r != hipSuccess) return r;
    }
    const int band = pf_band_rows(w), wpr = (w + 31) >> 5;
    const size_t lds = ((size_t)band * wpr + PF_WAVES * 3 + 3) * sizeof(uint32_t) & ~(size_t)15;
    const size_t plane = (size_t)h * w;
    for (int off = 0; off < n; off += PF_CHUNK) {
        const int m = n - off < PF_CHUNK ? n - off : PF_CHUNK;
        pf_fill_kernel<<<dim3((unsigned)((h + band - 1) / band), (unsigned)m), PF_THREADS, lds, s>>>(
            vertices, rings, table + (size_t)off * 5, h, w, x0, y0, masks_out ? masks_out + (size_t)off * plane : nullptr,
            ref ? ref + (size_t)off * plane : nullptr, counts_out ? (unsigned long long*)counts_out + (size_t)off * 3 : nullptr);
        const hipError_t r = hipGetLastError();
        if (r != hipSuccess) return r;
    }
    return hipSuccess;
}
