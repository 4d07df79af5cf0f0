// boundary_kernels.hip -- the boundary band of a mask, on its bit plane (gfx950): what Boundary IoU / Boundary AP (Cheng et al., CVPR
// 2021) count instead of the whole mask.  The definition (samrs_hip.h samrs_mask_boundary_bits states it):
//   band(M)[y][x] = M[y][x] AND NOT E[y][x],  E[y][x] = 1 iff every pixel of the (2 d + 1) x (2 d + 1) square centred on (y, x) lies
//   inside the image and is set in M  -- d iterations of a 3 x 3 all-ones erosion with a zero border.
// The square erosion is separable, and both passes work on the packed bits, 64 pixels per lane operation (boundary_word.h):
//   erode_rows_kernel   H = the horizontal pass.  A lane owns one output word; it loads the word and its one (d <= 64) or two
//                       neighbours on either side and ANDs shifted copies of that window, 1 + log2(2 d + 1) steps, then clears the
//                       bits whose window leaves the row.  Rows need not be word-aligned and a word may hold several rows: the
//                       window is a run of the flat bit string either way.
//   band_kernel         E = the vertical pass over H, then band = M & ~E.  The 2 d + 1 words at flat offsets p0 + k w are unaligned
//                       64-bit fetches, funnel-shifted from two words (one where w % 64 == 0); the bits whose window leaves the
//                       image are the complement of one flat range.  A lane whose mask word is empty has nothing to erode and a
//                       wave stops fetching once every lane's E is 0, which for a mask that covers little of its tile is at once.
//   For w < 2 d + 1 or h < 2 d + 1 no square fits: E is empty, the band is the mask and only band_kernel runs (`trivial`).
// One writer per output word, vector stores only, no atomics: the result is deterministic.  H is the only intermediate: scratch
// uint64 [n][words].
#include "common.h"
#include "kernels.h"
#include "boundary_word.h"

namespace {

typedef unsigned long long u64;

// lane t of grid.x: word t; grid.y strides over the masks
template <int NW>
__global__ __launch_bounds__(256) void erode_rows_kernel(const u64* __restrict__ planes, int n, long hw, long words, int w, int d,
                                                         u64* __restrict__ H) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    if (k >= words) return;
    const u64 valid = bw::row_valid(k * 64, hw, w, d);
    constexpr int C = NW / 2;
    for (int j = blockIdx.y; j < n; j += gridDim.y) {
        const u64* src = planes + (size_t)j * words;
        u64 out = 0ull;
        if (valid) {
            bw::Window<NW> win;
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                const long idx = k - C + i;
                win.v[i] = (idx >= 0 && idx < words) ? src[idx] : 0ull;
            }
            win.v[NW] = win.v[NW + 1] = win.v[NW + 2] = 0ull;
            out = bw::erode_row_word<NW>(win, d, valid);
        }
        H[(size_t)j * words + k] = out;
    }
}

// lane t of grid.x: word t; grid.y strides over the masks.  H is not read when `trivial`.
__global__ __launch_bounds__(256) void band_kernel(const u64* __restrict__ planes, const u64* __restrict__ H, int n, long hw, long words,
                                                   int w, int d, long y_lo, long y_hi, int trivial, u64* __restrict__ band) {
    const long k = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = k < words;
    const long p0 = k * 64;
    const u64 inside = live ? bw::range_bits(p0, 0, hw) : 0ull;
    const u64 yvalid = (live && !trivial) ? bw::range_bits(p0, y_lo, y_hi) : 0ull;       // d <= y < h - d
    for (int j = blockIdx.y; j < n; j += gridDim.y) {
        const u64 m = live ? planes[(size_t)j * words + k] & inside : 0ull;
        u64 e = m ? yvalid : 0ull;
        const u64* Hj = trivial ? planes : H + (size_t)j * words;                       // never read when trivial: e is 0
        for (int kk = -d; kk <= d; ++kk) {
            if (__ballot(e != 0ull) == 0ull) break;                                     // wave-uniform
            if (e) e &= bw::fetch_bits(Hj, words, p0 + (long)kk * w);
        }
        if (live) band[(size_t)j * words + k] = m & ~e;
    }
}

}  // namespace

size_t mask_boundary_scratch_bytes(int n, int h, int w) {
    return sizeof(u64) * (size_t)(n > 0 ? n : 1) * (size_t)(((long)h * w + 63) / 64);
}

hipError_t launch_mask_boundary(const unsigned long long* planes, int n, int h, int w, int d, void* scratch, unsigned long long* band_out,
                                hipStream_t s) {
    if (!planes || !band_out || n < 1 || h < 1 || w < 1 || d < 1 || d > 128 || (long)h * w >= (1l << 30)) return hipErrorInvalidValue;
    const long hw = (long)h * w, words = (hw + 63) / 64;
    const int trivial = (w < 2 * d + 1 || h < 2 * d + 1) ? 1 : 0;
    if (!trivial && !scratch) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((words + 255) / 256), (unsigned)(n < 65535 ? n : 65535));
    u64* H = (u64*)scratch;
    if (!trivial) {
        if (d <= 64)
            erode_rows_kernel<3><<<grid, 256, 0, s>>>(planes, n, hw, words, w, d, H);
        else
            erode_rows_kernel<5><<<grid, 256, 0, s>>>(planes, n, hw, words, w, d, H);
        HIP_CHECK_RET(hipGetLastError());
    }
    band_kernel<<<grid, 256, 0, s>>>(planes, H, n, hw, words, w, d, (long)d * w, (long)(h - d) * w, trivial, band_out);
    return hipGetLastError();
}
