// boundary_word.h -- the per-word arithmetic of boundary_kernels.hip, on 64 pixels of a bit plane at a time.  Plain integer C++ without
// any device intrinsic, so the same statements compile for the host (BW_HD empty) and can be checked there against a per-pixel erosion.
//
// A plane is one long bit string: pixel p = y w + x is bit p % 64 of word p / 64.  Within a row, x + k is flat p + k; a row below,
// p + w.  Both passes of the separable erosion therefore AND shifted copies of the string and clear the bits whose window leaves
// the image:
//   horizontal  H[p] = AND_{k = -d..d} M[p + k]      where d <= x < w - d, else 0
//   vertical    E[p] = AND_{k = -d..d} H[p + k w]    where d <= y < h - d, else 0     (these p are the flat range [d w, (h - d) w))
#pragma once
#include <cstdint>

#ifndef BW_HD
#define BW_HD __host__ __device__ __forceinline__
#endif

namespace bw {

typedef unsigned long long u64;

// the bits b of a word starting at flat pixel p0 with lo <= p0 + b < hi
BW_HD u64 range_bits(long p0, long lo, long hi) {
    const long a = lo - p0 > 0 ? lo - p0 : 0;
    const long b = hi - p0 < 64 ? hi - p0 : 64;
    if (a >= b) return 0ull;
    const u64 below_b = b == 64 ? ~0ull : ((1ull << b) - 1ull);
    return below_b & ~((1ull << a) - 1ull);
}

// the bits of that word whose pixel has d <= x < w - d: one interval per row the word touches (w >= 2 d + 1, so at most 64 / 3 + 2 rows)
BW_HD u64 row_valid(long p0, long hw, int w, int d) {
    u64 m = 0ull;
    const long end = p0 + 64 < hw ? p0 + 64 : hw;
    for (long row0 = p0 - p0 % w; row0 < end; row0 += w) m |= range_bits(p0, row0 + d, row0 + w - d);
    return m;
}

// v[i + j] for a compile-time i and a wave-uniform j in 0..2, as selects (a run-time index would put the window into scratch memory)
#define BW_SEL(v, i, j) ((j) == 0 ? (v)[(i)] : (j) == 1 ? (v)[(i) + 1] : (v)[(i) + 2])

// A window of NW words (64 NW bits, bit q of the window = flat pixel 64 (k - C) + q, C = NW / 2, for output word k), padded with three
// zero words so that every select above stays inside the array.
template <int NW>
struct Window {
    u64 v[NW + 3];

    // bit q &= bit q + s for every q of the window; zeros come in from above.  1 <= s <= 128
    BW_HD void and_shifted(int s) {
        const int j = s >> 6, r = s & 63;
#pragma unroll
        for (int i = 0; i < NW; ++i) {                   // ascending: word i only reads words >= i
            const u64 lo = BW_SEL(v, i, j), hi = BW_SEL(v, i + 1, j);
            v[i] &= r ? ((lo >> r) | (hi << (64 - r))) : lo;
        }
    }
    // the 64 bits from window bit `off` on, 0 <= off < 128
    BW_HD u64 extract(int off) const {
        const int j = off >> 6, r = off & 63;
        const u64 lo = BW_SEL(v, 0, j), hi = BW_SEL(v, 1, j);
        return r ? ((lo >> r) | (hi << (64 - r))) : lo;
    }
};

// Word k of H from the NW words around word k of M (already loaded into win.v[0 .. NW), words outside the plane as 0; NW = 3 serves
// d <= 64, NW = 5 d <= 128).  R_s[q] = AND of the s bits from q on: R_1 = M, R_2s[q] = R_s[q] & R_s[q + s], and for the window length
// L = 2 d + 1 with a the greatest power of two <= L, R_L[q] = R_a[q] & R_a[q + L - a] (L - a < a: the two runs overlap or touch).  H[p]
// = R_L[p - d].  R_s[q] is right wherever q + s - 1 is inside the window, and the output's bits need q + L - 1 = p + d <= 64 C + 63 + d,
// which is: 1 + log2(L) shift-and-AND steps over NW words.
template <int NW>
BW_HD u64 erode_row_word(Window<NW>& win, int d, u64 valid) {
    const int L = 2 * d + 1;
    int s = 1;
    for (; 2 * s <= L; s *= 2) win.and_shifted(s);
    if (s < L) win.and_shifted(L - s);
    return win.extract(64 * (NW / 2) - d) & valid;
}

// the 64 bits of plane P [words] from flat pixel q on (q may be negative or past the end: words outside the plane read as 0).  The
// shift q & 63 is the same for every word of a launch step, so the branch on it is wave-uniform; rows of a multiple of 64 pixels
// take one load.
BW_HD u64 fetch_bits(const u64* __restrict__ P, long words, long q) {
    const long i = q >> 6;                               // floor, also for q < 0
    const int r = (int)(q & 63);
    const u64 lo = (i >= 0 && i < words) ? P[i] : 0ull;
    if (r == 0) return lo;
    const u64 hi = (i + 1 >= 0 && i + 1 < words) ? P[i + 1] : 0ull;
    return (lo >> r) | (hi << (64 - r));
}

}  // namespace bw
