// rle_decode_kernels.hip -- COCO run-length DEcoding on the device (gfx950): the inverse of rle_kernels.hip.
//
// Reads what samrs_rle_encode writes (and what cocoapi's rleToString writes): per mask an ASCII string of delta-coded 5-bit groups
// (cocoapi rleFrString: char - 48, bit 5 = "more groups follow", bit 4 of the last group sign-extends, from the 4th count on a delta
// against the count two back), counts = column-major runs starting with zeros.  Out: row-major 0 / 1 bytes [n][H][W] + areas + a
// status per mask.  The strings are untrusted bytes: every index that depends on them is range-checked before it reaches memory,
// sums are taken in 64 bits, and a mask is filled only when its whole string validated (status 0); the fill clamps to H W anyway.
//
// Byte / integer work, per batch of m <= 32 masks, RLED_NB blocks per mask in the string passes (the host does not know the strings'
// lengths: the table is device memory, so a block loops over its share in tiles):
//   0. rled_prep_kernel     (offset, length) of the table checked against the buffer -> ABSENT / RANGE / the empty string; the masks'
//                           tokens are packed into ONE int32 array of `cap` = strings_bytes entries, mask j behind the lengths before it.
//   1. rled_tokens_kernel   twice (count, then write): byte i starts a token iff i == 0 or byte i - 1 has no continuation bit; block scan
//                           -> token index; the thread at a token start assembles <= 7 groups into a delta.  BAD_CHAR / TRUNCATED /
//                           more than 7 chars are OR-ed into the mask's flag word (integer atomics: order-free).
//   2. rled_chain_kernel    twice (block sums, then write): c[k] = d[k] + c[k - 2] (k >= 3) = two interleaved inclusive scans, a thread
//                           owns the pair (2t, 2t + 1): the even chain from k = 2, the odd chain from k = 1, c[0] alone.  In place, 64-bit
//                           sums; c < 0 -> BAD_COUNT, c > H W -> BAD_SUM.
//   3. rled_bounds_kernel   B[k] = sum_{j <= k} c[j], in place (the block sums of c come from pass 2).
//   4. rled_status_kernel   B[last] != H W -> BAD_SUM; status = the lowest code flagged.
//   5. rled_fill_kernel     the encoder's column-major bit matrix [m][W][ceil(H/32)], thread = word: upper-bound search of the word's
//                           first position in B -> run index (its parity is the pixel value), then the boundaries inside the word.
//   6. rled_unpack_kernel   mirror of rle_bitpack_kernel: bit matrix -> row-major bytes, a lane owns 4 columns x 128 rows, 16-byte
//                           column reads, coalesced 4-byte row stores; areas = popcount + wave reduce + one integer atomic per wave.
// Every cross-block dependence is a kernel boundary (no grid barriers, no spin-waits): the result does not depend on scheduling.
// Integer arithmetic only: bit-exact with samrs_amd/rle.py:decode (tests/test_rle_decode_gpu.py).
#include "common.h"
#include "kernels.h"

namespace {

constexpr int RLED_THREADS = 1024;
constexpr int RLED_NB = 16;                     // blocks per mask of the string / count passes
constexpr int RLED_MAX = 32;                    // masks per launch (the prep and status kernels are one block)

enum : uint32_t {                               // flag bit = 1 << status code (samrs_rle_status)
    F_ABSENT = 1u << 1, F_RANGE = 1u << 2, F_BAD_CHAR = 1u << 3, F_TRUNCATED = 1u << 4, F_BAD_COUNT = 1u << 5, F_BAD_SUM = 1u << 6
};

struct RledMeta {                               // per mask of the batch, written by the prep kernel
    long long off;                              // first byte of the string in `strings` (0 when not usable)
    uint32_t len;                               // bytes to read (0 when not usable: nothing of the string is touched)
    uint32_t base;                              // first entry of the mask's tokens in the token array; base + len <= cap
};

// scratch counters of a batch (after the token array and the bit matrix)
struct RledCtr {
    RledMeta meta[RLED_MAX];
    uint32_t flags[RLED_MAX];
    uint32_t ntok[RLED_MAX];
    int32_t status[RLED_MAX];
    uint32_t blk_tok[RLED_MAX][RLED_NB];        // tokens per block (pass 1)
    long long blk_chain[RLED_MAX][RLED_NB][2];  // sums of the even / odd deltas per block (pass 2)
    long long blk_sum[RLED_MAX][RLED_NB];       // sums of the counts per block (pass 2 -> 3)
};

__device__ __forceinline__ bool rled_cont(int ch) { return ((ch - 48) & 0x20) != 0; }

// inclusive block scan of one 64-bit value per thread (RLED_THREADS threads); *total = sum.  sm: 17 entries.
__device__ __forceinline__ long long rled_scan_incl(long long v, long long* sm, long long* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    __syncthreads();                       // sm free (previous use)
    if (lane == 63) sm[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int i = 0; i < RLED_THREADS / 64; ++i) { const long long t = sm[i]; sm[i] = run; run += t; }
        sm[16] = run;
    }
    __syncthreads();
    *total = sm[16];
    return sm[wave] + inc;
}

// one block.  Decides what can be decided from the table alone and lays the masks' token ranges out.
__global__ void rled_prep_kernel(const long long* __restrict__ table, int m, long long strings_bytes, uint32_t cap, RledCtr* __restrict__ ctr,
                                 unsigned long long* __restrict__ areas /* or null */) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    uint32_t run = 0;
    for (int j = 0; j < m; ++j) {
        const long long off = table[3 * j], len = table[3 * j + 1];
        uint32_t f = 0;
        if (len < 0) f = F_ABSENT;
        else if (off < 0 || off > strings_bytes || len > strings_bytes - off) f = F_RANGE;
        else if (len == 0) f = F_BAD_SUM;                                  // the empty string: no counts, sum 0 != h w
        else if (len > (long long)(cap - run)) f = F_RANGE;                // entries that together name more bytes than the buffer holds
        RledMeta mt;
        mt.off = f ? 0 : off;
        mt.len = f ? 0u : (uint32_t)len;
        mt.base = run;
        run += mt.len;
        ctr->meta[j] = mt;
        ctr->flags[j] = f;
        ctr->ntok[j] = 0;
        if (areas) areas[j] = 0ull;
    }
}

// grid (RLED_NB, m).  WRITE = false: tokens per block.  WRITE = true: the deltas, saturated to int32 (a delta outside int32 makes its
// count negative or larger than 2^30 either way), into tok[base + token index]; token index < len, so the store is inside the mask's range.
template <bool WRITE>
__global__ __launch_bounds__(RLED_THREADS) void rled_tokens_kernel(const uint8_t* __restrict__ strings, int32_t* __restrict__ tok,
                                                                   RledCtr* __restrict__ ctr) {
    __shared__ long long sm[17];
    const int j = blockIdx.y, blk = blockIdx.x;
    const RledMeta mt = ctr->meta[j];
    const uint32_t L = mt.len;
    if (L == 0) return;                                                    // uniform per block
    const uint8_t* s = strings + mt.off;
    const uint32_t per = ((L + RLED_NB - 1) / RLED_NB + RLED_THREADS - 1) & ~(uint32_t)(RLED_THREADS - 1);
    const uint32_t i0 = (uint64_t)blk * per < L ? blk * per : L, i1 = L - i0 < per ? L : i0 + per;
    uint32_t carry = 0, flags = 0;
    if (WRITE)
        for (int b = 0; b < blk; ++b) carry += ctr->blk_tok[j][b];
    for (uint32_t t0 = i0; t0 < i1; t0 += RLED_THREADS) {
        const uint32_t i = t0 + threadIdx.x;
        const bool in = i < i1;
        const int ch = in ? (int)s[i] : 48;
        if (in && (ch < 48 || ch > 111)) flags |= F_BAD_CHAR;
        if (in && i == L - 1 && rled_cont(ch)) flags |= F_TRUNCATED;
        const bool start = in && (i == 0 || !rled_cont((int)s[i - 1]));
        long long total;
        const long long incl = rled_scan_incl(start ? 1 : 0, sm, &total);
        if (WRITE && start) {
            long long x = 0;
            int g = 0;
            bool more = true;
            int c = 0;
            while (more && g < 7 && i + g < L) {
                c = (int)s[i + g] - 48;
                x |= (long long)(c & 0x1f) << (5 * g);
                more = (c & 0x20) != 0;
                ++g;
            }
            if (more && g == 7) flags |= F_BAD_COUNT;                      // a token of more than 7 chars
            if (!more && (c & 0x10)) x |= -1ll << (5 * g);
            x = x > 2147483647ll ? 2147483647ll : (x < -2147483648ll ? -2147483648ll : x);
            const uint32_t k = carry + (uint32_t)incl - 1u;               // < L: tokens <= bytes
            if (k < L) tok[(size_t)mt.base + k] = (int32_t)x;
        }
        carry += (uint32_t)total;
    }
    if (flags) atomicOr(&ctr->flags[j], flags);
    if (!WRITE) {
        if (threadIdx.x == 0) ctr->blk_tok[j][blk] = carry;
    } else if (blk == RLED_NB - 1 && threadIdx.x == 0) {
        ctr->ntok[j] = carry < L ? carry : L;
    }
}

// grid (RLED_NB, m).  A thread owns the token pair (2t, 2t + 1) of a tile of 2 RLED_THREADS tokens; block ranges are whole tiles, so a
// token's parity in its tile is its parity in the mask.  PASS 0: the block's sums of the even (k >= 2) and odd deltas.  PASS 1: the
// counts, in place, and the block's sum of them.  PASS 2: the boundaries, in place.
template <int PASS>
__global__ __launch_bounds__(RLED_THREADS) void rled_chain_kernel(int32_t* __restrict__ tok, RledCtr* __restrict__ ctr, long long HW) {
    __shared__ long long sm[17];
    const int j = blockIdx.y, blk = blockIdx.x;
    const uint32_t nt = ctr->ntok[j];
    if (nt == 0) return;                                                   // uniform per block
    int32_t* a = tok + (size_t)ctr->meta[j].base;                          // nt <= len entries
    constexpr uint32_t TILE = 2 * RLED_THREADS;
    const uint32_t per = ((nt + RLED_NB - 1) / RLED_NB + TILE - 1) & ~(TILE - 1);
    const uint32_t k0 = (uint64_t)blk * per < nt ? blk * per : nt, k1 = nt - k0 < per ? nt : k0 + per;
    long long ce = 0, co = 0, cs = 0;                                      // carries: even chain, odd chain, boundary sum
    uint32_t flags = 0;
    if (PASS == 1)
        for (int b = 0; b < blk; ++b) { ce += ctr->blk_chain[j][b][0]; co += ctr->blk_chain[j][b][1]; }
    if (PASS == 2)
        for (int b = 0; b < blk; ++b) cs += ctr->blk_sum[j][b];
    long long sum_c = 0;
    for (uint32_t t0 = k0; t0 < k1; t0 += TILE) {
        const uint32_t ka = t0 + 2 * threadIdx.x, kb = ka + 1;
        const bool ina = ka < k1, inb = kb < k1;
        const long long va = ina ? (long long)a[ka] : 0, vb = inb ? (long long)a[kb] : 0;
        if (PASS == 2) {
            // counts were stored as 0 .. HW + 1 (uint32 in an int32 slot)
            const long long ca = (long long)(uint32_t)va, cb = (long long)(uint32_t)vb;
            long long total;
            const long long incl = rled_scan_incl(ca + cb, sm, &total);
            const long long bb = cs + incl, ba = bb - cb;
            const long long lim = HW + 1;                                  // a dead mask's sums are clamped; it is never filled
            if (ina) a[ka] = (int32_t)(uint32_t)(ba > lim ? lim : ba);
            if (inb) a[kb] = (int32_t)(uint32_t)(bb > lim ? lim : bb);
            cs += total;
        } else {
            long long te, to;
            const long long ie = rled_scan_incl(ka == 0 ? 0 : va, sm, &te);      // c[0] stands alone
            const long long io = rled_scan_incl(vb, sm, &to);
            if (PASS == 1) {
                long long ca = ka == 0 ? va : ce + ie, cb = co + io;
                if (ina && ca < 0) { flags |= F_BAD_COUNT; ca = 0; }
                if (inb && cb < 0) { flags |= F_BAD_COUNT; cb = 0; }
                if (ina && ca > HW) { flags |= F_BAD_SUM; ca = HW + 1; }
                if (inb && cb > HW) { flags |= F_BAD_SUM; cb = HW + 1; }
                if (ina) { a[ka] = (int32_t)(uint32_t)ca; sum_c += ca; }
                if (inb) { a[kb] = (int32_t)(uint32_t)cb; sum_c += cb; }
            }
            ce += te;
            co += to;
        }
    }
    if (PASS == 0) {
        if (threadIdx.x == 0) { ctr->blk_chain[j][blk][0] = ce; ctr->blk_chain[j][blk][1] = co; }
    } else if (PASS == 1) {
        if (flags) atomicOr(&ctr->flags[j], flags);
        long long total;
        rled_scan_incl(sum_c, sm, &total);
        if (threadIdx.x == 0) ctr->blk_sum[j][blk] = total;
    }
}

// one block, thread = mask: the sum check and the status (the lowest code flagged)
__global__ void rled_status_kernel(RledCtr* __restrict__ ctr, int m, long long HW, int32_t* __restrict__ status_out) {
    const int j = threadIdx.x;
    if (blockIdx.x != 0 || j >= m) return;
    uint32_t f = ctr->flags[j];
    if (ctr->ntok[j] > 0) {
        long long total = 0;
        for (int b = 0; b < RLED_NB; ++b) total += ctr->blk_sum[j][b];   // <= RLED_NB * 2^21 * (2^30 + 1): no overflow
        if (total != HW) f |= F_BAD_SUM;
    } else if (f == 0) {
        f = F_BAD_SUM;
    }
    const int st = f ? __ffs((int)f) - 1 : 0;
    ctr->status[j] = st;
    status_out[j] = st;
}

// grid (ceil(W YW / 256), m), thread = word (column x, rows 32 yw .. + 31).  Pixel p = x H + y is set iff the number of boundaries <= p
// is odd.  Words of a mask that did not validate are zero.
__global__ __launch_bounds__(256) void rled_fill_kernel(const int32_t* __restrict__ tok, const RledCtr* __restrict__ ctr,
                                                        uint32_t* __restrict__ bits, int H, int W, int YW) {
    const int j = blockIdx.y;
    const size_t wi = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (wi >= (size_t)W * YW) return;
    uint32_t word = 0u;
    if (ctr->status[j] == 0) {
        const uint32_t* B = reinterpret_cast<const uint32_t*>(tok) + (size_t)ctr->meta[j].base;
        const uint32_t nt = ctr->ntok[j];
        const uint32_t HW = (uint32_t)H * (uint32_t)W;
        const int x = (int)(wi / YW), yw = (int)(wi % YW);
        const uint32_t p0 = (uint32_t)x * (uint32_t)H + 32u * yw;
        const uint32_t nb = H - 32 * yw < 32 ? (uint32_t)(H - 32 * yw) : 32u;
        const uint32_t end = p0 + nb;                                      // <= H W
        uint32_t lo = 0, hi = nt;                                          // first r with B[r] > p0
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (B[mid] <= p0) lo = mid + 1; else hi = mid;
        }
        uint32_t r = lo, cur = p0;
        while (cur < end) {
            uint32_t b = r < nt ? B[r] : HW;
            b = b < cur ? cur : (b > end ? end : b);                       // clamped to the word (B ascends: a no-op for a valid mask)
            if ((r & 1u) && b > cur) {
                const uint32_t n1 = b - cur, s0 = cur - p0;                // 1 <= n1 <= 32, s0 + n1 <= 32
                word |= (n1 == 32u ? 0xFFFFFFFFu : ((1u << n1) - 1u)) << s0;
            }
            if (r >= nt) break;
            cur = b;
            if (b == end) break;
            ++r;
        }
    }
    bits[(size_t)j * W * YW + wi] = word;
}

// grid (ceil(H / 128), m, ceil(W / 1024)), 256 threads.  Thread t: columns x0 + 4t .. +3, rows y0 .. y0 + 127 (rle_bitpack_kernel's
// tiling, backwards).  Every byte of the mask is written.
__global__ __launch_bounds__(256) void rled_unpack_kernel(const uint32_t* __restrict__ bits, uint8_t* __restrict__ masks,
                                                          unsigned long long* __restrict__ areas /* or null */, int H, int W, int YW) {
    const int m = blockIdx.y;
    const int x = blockIdx.z * 1024 + threadIdx.x * 4;
    const int y0 = blockIdx.x * 128;
    const int yw0 = blockIdx.x * 4;
    uint8_t* dst = masks + (size_t)m * H * W;
    uint32_t w[4][4];
    uint32_t cnt = 0;
    if (x < W) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
            for (int r = 0; r < 4; ++r) w[c][r] = 0u;
            if (x + c >= W) continue;
            const uint32_t* src = bits + ((size_t)m * W + x + c) * YW + yw0;
            if (yw0 + 4 <= YW && (YW & 3) == 0) {
                const uint4 q = *reinterpret_cast<const uint4*>(src);
                w[c][0] = q.x; w[c][1] = q.y; w[c][2] = q.z; w[c][3] = q.w;
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (yw0 + r < YW) w[c][r] = src[r];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) cnt += __popc(w[c][r]);
        }
        const bool wide = (W & 3) == 0 && (((uintptr_t)dst) & 3) == 0;    // whole 4-byte words of a row
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll 8
            for (int b = 0; b < 32; ++b) {
                const int y = y0 + 32 * r + b;
                if (y >= H) break;
                uint32_t px = 0u;
#pragma unroll
                for (int c = 0; c < 4; ++c) px |= ((w[c][r] >> b) & 1u) << (8 * c);
                if (wide) {
                    *reinterpret_cast<uint32_t*>(dst + (size_t)y * W + x) = px;
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (x + c < W) dst[(size_t)y * W + x + c] = (uint8_t)((px >> (8 * c)) & 1u);
                }
            }
        }
    }
    if (areas) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&areas[m], (unsigned long long)cnt);
    }
}

inline size_t rled_align(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

int rle_decode_max_batch() { return RLED_MAX; }

size_t rle_decode_scratch_bytes(int n, int h, int w, long long strings_bytes) {
    const size_t yw = (size_t)(h + 31) / 32;
    return rled_align((size_t)strings_bytes * 4) + rled_align((size_t)n * w * yw * 4) + rled_align(sizeof(RledCtr));
}

hipError_t launch_rle_decode(const uint8_t* strings, long long strings_bytes, const long long* table, int n, int h, int w, void* scratch,
                             uint8_t* masks_out, long long* areas_out, int32_t* status_out, hipStream_t s) {
    if (n < 1 || n > RLED_MAX || h < 1 || w < 1 || (size_t)h * w >= (1ull << 30) || strings_bytes < 0 || strings_bytes >= (1ll << 31))
        return hipErrorInvalidValue;
    const int YW = (h + 31) / 32;
    unsigned char* p = reinterpret_cast<unsigned char*>(scratch);
    int32_t* tok = reinterpret_cast<int32_t*>(p);
    p += rled_align((size_t)strings_bytes * 4);
    uint32_t* bits = reinterpret_cast<uint32_t*>(p);
    p += rled_align((size_t)n * w * YW * 4);
    RledCtr* ctr = reinterpret_cast<RledCtr*>(p);
    const long long HW = (long long)h * w;
    unsigned long long* areas = reinterpret_cast<unsigned long long*>(areas_out);
    rled_prep_kernel<<<1, 64, 0, s>>>(table, n, strings_bytes, (uint32_t)strings_bytes, ctr, areas);
    rled_tokens_kernel<false><<<dim3(RLED_NB, n), RLED_THREADS, 0, s>>>(strings, tok, ctr);
    rled_tokens_kernel<true><<<dim3(RLED_NB, n), RLED_THREADS, 0, s>>>(strings, tok, ctr);
    rled_chain_kernel<0><<<dim3(RLED_NB, n), RLED_THREADS, 0, s>>>(tok, ctr, HW);
    rled_chain_kernel<1><<<dim3(RLED_NB, n), RLED_THREADS, 0, s>>>(tok, ctr, HW);
    rled_chain_kernel<2><<<dim3(RLED_NB, n), RLED_THREADS, 0, s>>>(tok, ctr, HW);
    rled_status_kernel<<<1, 64, 0, s>>>(ctr, n, HW, status_out);
    rled_fill_kernel<<<dim3((unsigned)(((size_t)w * YW + 255) / 256), n), 256, 0, s>>>(tok, ctr, bits, h, w, YW);
    rled_unpack_kernel<<<dim3((h + 127) / 128, n, (w + 1023) / 1024), 256, 0, s>>>(bits, masks_out, areas, h, w, YW);
    return hipGetLastError();
}
