// png_kernels.hip -- the generation CLI's gray/<stem>.png and color/<stem>.png of a class map, encoded on the device (gfx950).
//
// Byte-identical with the host's label-aware pair writer (io_png.cc: encode_labels -> parse_labels (unit 3) -> emit_labels for
// bpp 1 and bpp 3): one greedy parse of the label map into pixel-unit tokens shared by both streams, one dynamic-Huffman deflate
// block per 2^20 parse tokens, plain Huffman lengths under the strict (weight, node index) order with the halve-and-rebuild
// length limit, canonical codes written LSB first; zlib header 78 9c, Adler-32 of the filter-0 rows, PNG framing with CRC-32.
//
// Per pass of up to PNG_MAPS maps (sizes stay on the device; every grid is sized for the worst case and idle blocks return):
//   1. png_parse_kernel      thread = row: the host's greedy walk, tokens into a per-row slot of w + 1 entries + the row's count
//   2. png_scan_rows_kernel  block = map: row counts -> row offsets, token / block / chunk counts
//   3. png_compact_kernel    block = row: slot -> the map's contiguous token list
//   4. png_hist_kernel       block = 1024 tokens (a chunk; 2^10 chunks per deflate block): both streams' literal / length and
//                            distance histograms, LDS atomics, then integer atomics into the block's histogram (order-free sums)
//   5. png_tables_kernel     wave = (deflate block, stream): Huffman lengths, canonical codes, the block header's bits
//   6. png_tokbits_kernel    block = chunk: bits of every token in both streams -> per-chunk bit counts
//   7. png_scan_chunks_kernel block = (map, stream): chunk bit offsets; header / end-of-block gaps in front of each block's first chunk
//   8. png_place_kernel      one thread: file lengths -> 16-byte aligned offsets behind *cursor, (offset, length) table, cursor
//   9. png_zero_kernel       the files' byte ranges are zeroed
//  10. png_pack_kernel       block = (chunk, stream): the chunk's bits assembled in LDS (bit ranges of tokens are disjoint), whole
//                            words stored, the two edge words OR-ed (shared with the neighbours)
//  11. png_headers_kernel    wave = (block boundary, stream): end-of-block code of the previous block + this block's header, OR-ed
//  12. png_adler_rows_kernel wave = (row, stream): the row's byte sum and position-weighted sum (mod 65521)
//  13. png_frame_kernel      wave = (map, stream): Adler-32 = combination of the row sums; signature, IHDR, IDAT head, zlib header,
//                            Adler, IEND
//  14. png_crc_kernel        thread = 256 bytes of IDAT: CRC register contribution shifted to the end of the chunk (GF(2)
//                            multiplication by x^(8 k) mod P, as zlib's crc32_combine), XOR-reduced (order-free)
//  15. png_crc_finish_kernel the IDAT CRC.
// Integer work only; every cross-block dependence is a kernel boundary and every atomic is an order-free integer sum / OR / XOR:
// the bytes do not depend on scheduling.
// Stages 5, 7, 9, 11, 14 and 15 look at no token: png_stage_* (kernels.h, at the end of this file) launch them for overlay_kernels.hip's
// truecolour encoder too, whose symbols are filtered bytes, for stream 0 of each slot.  The helpers both sources use: png_device.h.
#include "common.h"
#include "kernels.h"
#include "png_device.h"

namespace {

constexpr int PNG_TOKEN_BITS = 144;              // most bits of one token: 3 colour matches of (15 + 5) + (15 + 13) bits
constexpr int PNG_PACK_WORDS = (PNG_CHUNK * PNG_TOKEN_BITS + 31) / 32 + 2;
// the constants of the scratch layout, the meta block and the helpers both device encoders use: png_device.h

// token (uint32): 0 = the row's filter byte; 0x40000000 | label = a literal pixel;
// 0x80000000 | up << 29 | v1 << 17 | v0 << 9 | npx = a run of npx (1 .. 258) pixels equal to the row above (up) or to the left
// neighbour; v0 / v1 = the labels at the run's first two pixels (the gray stream writes runs of 1 or 2 pixels as literals)
__constant__ uint16_t kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131,
                                      163, 195, 227, 258};
__constant__ uint8_t kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
                                       2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
__constant__ uint8_t kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ int len_code(int len) {              // 3 .. 258 -> 0 .. 28
    int c = 28;
    while (kLenBase[c] > len) --c;
    return c;
}
__device__ __forceinline__ int dist_code(int dist) {
    int c = 29;
    while (kDistBase[c] > dist) --c;
    return c;
}

struct Layout {                                   // scratch of one pass, carved from the engine's PNG scratch buffer
    uint32_t *slot, *tok, *rowcnt, *rowoff, *hist, *tables, *hdr, *hdrbits, *chunkbits, *adler;
    unsigned long long *meta, *chunkoff, *gapoff;
    size_t T, C, B;                               // worst-case tokens, chunks, deflate blocks per map
};

// base == nullptr: only *bytes is computed.  Every piece starts 256-byte aligned.
Layout carve(void* base, int nm, int h, int w, size_t* bytes) {
    Layout L;
    L.T = (size_t)h * (w + 1);
    L.C = (L.T + PNG_CHUNK - 1) / PNG_CHUNK;
    L.B = (L.T + (1u << PNG_BLOCK_SHIFT) - 1) >> PNG_BLOCK_SHIFT;
    unsigned char* p = static_cast<unsigned char*>(base);
    size_t used = 0;
    auto take = [&](size_t n) { unsigned char* q = p ? p + used : nullptr; used += align256(n); return q; };
    L.meta = reinterpret_cast<unsigned long long*>(take((size_t)nm * MT_N * 8));
    L.hist = reinterpret_cast<uint32_t*>(take((size_t)nm * L.B * 2 * PNG_NSYM * 4));
    L.slot = reinterpret_cast<uint32_t*>(take((size_t)nm * L.T * 4));
    L.tok = reinterpret_cast<uint32_t*>(take((size_t)nm * L.T * 4));
    L.rowcnt = reinterpret_cast<uint32_t*>(take((size_t)nm * h * 4));
    L.rowoff = reinterpret_cast<uint32_t*>(take((size_t)nm * h * 4));
    L.tables = reinterpret_cast<uint32_t*>(take((size_t)nm * L.B * 2 * PNG_NSYM * 4));
    L.hdr = reinterpret_cast<uint32_t*>(take((size_t)nm * L.B * 2 * PNG_HDR_WORDS * 4));
    L.hdrbits = reinterpret_cast<uint32_t*>(take((size_t)nm * L.B * 2 * 4));
    L.chunkbits = reinterpret_cast<uint32_t*>(take((size_t)nm * 2 * L.C * 4));
    L.chunkoff = reinterpret_cast<unsigned long long*>(take((size_t)nm * 2 * L.C * 8));
    L.gapoff = reinterpret_cast<unsigned long long*>(take((size_t)nm * 2 * (L.B + 1) * 8));
    L.adler = reinterpret_cast<uint32_t*>(take((size_t)nm * 2 * h * 8));
    if (bytes) *bytes = used;
    return L;
}

// ---- 1. parse ----------------------------------------------------------------------------------------------------------------
// the host's parse_labels for unit 3 (min 1 pixel, up_bias 1, <= 258 pixels per token); grid (ceil(h / 64), nm), 64 threads
__global__ __launch_bounds__(64) void png_parse_kernel(const uint8_t* __restrict__ maps, uint32_t* __restrict__ slot,
                                                       uint32_t* __restrict__ rowcnt, int h, int w, int up_ok, size_t T) {
    const int m = blockIdx.y, y = blockIdx.x * 64 + threadIdx.x;
    if (y >= h) return;
    const uint8_t* g = maps + ((size_t)m * h + y) * w;
    const uint8_t* up = (y > 0 && up_ok) ? g - w : nullptr;
    uint32_t* t = slot + (size_t)m * T + (size_t)y * (w + 1);
    uint32_t cnt = 0;
    t[cnt++] = 0u;                                   // the filter-type byte
    int x = 0;
    while (x < w) {
        int lu = 0, ll = 0;
        if (up) while (x + lu < w && g[x + lu] == up[x + lu]) ++lu;
        if (x > 0) while (x + ll < w && g[x + ll] == g[x + ll - 1]) ++ll;
        int n = 0;
        uint32_t upf = 0;
        if (lu >= 1 && lu > ll + 1) { n = lu; upf = 1; }
        else if (ll >= 1) n = ll;
        else if (lu >= 1) { n = lu > 258 ? 258 : lu; upf = 1; }
        if (!n) { t[cnt++] = 0x40000000u | g[x]; ++x; continue; }
        while (n > 0) {
            const int k = n > 258 ? 258 : n;
            uint32_t v = 0x80000000u | (upf << 29) | (uint32_t)k;
            if (k <= 2) v |= ((uint32_t)g[x] << 9) | ((uint32_t)g[x + 1 < w ? x + 1 : x] << 17);
            t[cnt++] = v;
            x += k; n -= k;
        }
    }
    rowcnt[(size_t)m * h + y] = cnt;
}

// ---- 2. row offsets ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void png_scan_rows_kernel(const uint32_t* __restrict__ rowcnt, uint32_t* __restrict__ rowoff,
                                                             unsigned long long* __restrict__ meta, int h) {
    __shared__ uint32_t sm[17];
    const int m = blockIdx.x;
    uint32_t carry = 0;
    for (int y0 = 0; y0 < h; y0 += 1024) {
        const int y = y0 + threadIdx.x;
        const uint32_t v = y < h ? rowcnt[(size_t)m * h + y] : 0u;
        uint32_t tot;
        const uint32_t ex = block_scan_excl(v, sm, &tot);
        if (y < h) rowoff[(size_t)m * h + y] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) {
        unsigned long long* mt = meta + (size_t)m * MT_N;
        mt[MT_NTOK] = carry;
        mt[MT_NBLK] = (carry + (1u << PNG_BLOCK_SHIFT) - 1) >> PNG_BLOCK_SHIFT;
        mt[MT_NCHUNK] = (carry + PNG_CHUNK - 1) / PNG_CHUNK;
    }
}

// ---- 3. compact --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void png_compact_kernel(const uint32_t* __restrict__ slot, const uint32_t* __restrict__ rowcnt,
                                                          const uint32_t* __restrict__ rowoff, uint32_t* __restrict__ tok, int h,
                                                          int w, size_t T) {
    const int m = blockIdx.y, y = blockIdx.x;
    const uint32_t cnt = rowcnt[(size_t)m * h + y], off = rowoff[(size_t)m * h + y];
    const uint32_t* s = slot + (size_t)m * T + (size_t)y * (w + 1);
    uint32_t* d = tok + (size_t)m * T + off;
    for (uint32_t i = threadIdx.x; i < cnt; i += 256) d[i] = s[i];
}

// ---- token -> symbols / bits -------------------------------------------------------------------------------------------------
struct DistInfo { int left_sym, up_sym, up_ebits, up_eval; };

__host__ __device__ inline int dist_code_host(int dist) {      // same as dist_code, usable from the launch code
    const int base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
                          4097, 6145, 8193, 12289, 16385, 24577};
    int c = 29;
    while (base[c] > dist) --c;
    return c;
}

__device__ __forceinline__ DistInfo dist_info(int s, int w, int up_ok) {
    DistInfo d;
    d.left_sym = dist_code(s ? 3 : 1);            // left: bpp bytes back, no extra bits (codes 2 / 0)
    const int du = s ? 3 * w + 1 : w + 1;
    if (up_ok) { d.up_sym = dist_code(du); d.up_ebits = kDistExtra[d.up_sym]; d.up_eval = du - kDistBase[d.up_sym]; }
    else { d.up_sym = 0; d.up_ebits = 0; d.up_eval = 0; }
    return d;
}

// the symbols of one token in stream s: lit(sym) for a literal / length symbol, dist(sym) for a distance symbol
template <class Lit, class Len, class Dist>
__device__ __forceinline__ void token_symbols(uint32_t k, int s, const uint32_t* __restrict__ lut32, const DistInfo& di, Lit&& lit,
                                              Len&& len, Dist&& dist) {
    if (!(k >> 30)) { lit(0u); return; }                                // filter byte 0
    if (!(k >> 31)) {                                                   // literal pixel
        const uint32_t lab = k & 0xff;
        if (s == 0) lit(lab);
        else { const uint32_t c = lut32[lab]; lit(c & 0xff); lit((c >> 8) & 0xff); lit((c >> 16) & 0xff); }
        return;
    }
    const int n = (int)(k & 0x1ff);
    const bool upf = (k >> 29) & 1;
    if (s == 0) {
        if (n < 3) { lit((k >> 9) & 0xff); if (n == 2) lit((k >> 17) & 0xff); return; }
        len(n);
        dist(upf);
        return;
    }
    for (int r = n; r > 0;) {
        const int p = r > 86 ? 86 : r;
        len(p * 3);
        dist(upf);
        r -= p;
    }
}

// ---- 4. histograms -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_lut32(const uint8_t* __restrict__ lut, uint32_t* lut32) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x)
        lut32[i] = (uint32_t)lut[3 * i] | ((uint32_t)lut[3 * i + 1] << 8) | ((uint32_t)lut[3 * i + 2] << 16);
}

// grid (C, nm), 1024 threads
__global__ __launch_bounds__(1024) void png_hist_kernel(const uint32_t* __restrict__ tok, const unsigned long long* __restrict__ meta,
                                                        const uint8_t* __restrict__ lut, uint32_t* __restrict__ hist, int w,
                                                        int up_ok, size_t T, size_t B) {
    __shared__ uint32_t hs[2][PNG_NSYM];
    __shared__ uint32_t lut32[256];
    const int m = blockIdx.y, c = blockIdx.x;
    const unsigned long long* mt = meta + (size_t)m * MT_N;
    if ((unsigned long long)c >= mt[MT_NCHUNK]) return;
    for (int i = threadIdx.x; i < 2 * PNG_NSYM; i += blockDim.x) (&hs[0][0])[i] = 0u;
    load_lut32(lut, lut32);
    __syncthreads();
    const size_t g = (size_t)c * PNG_CHUNK + threadIdx.x;
    if (g < mt[MT_NTOK]) {
        const uint32_t k = tok[(size_t)m * T + g];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const DistInfo di = dist_info(s, w, up_ok);
            token_symbols(k, s, lut32, di,
                          [&](uint32_t sym) { atomicAdd(&hs[s][sym], 1u); },
                          [&](int l) { atomicAdd(&hs[s][257 + len_code(l)], 1u); },
                          [&](bool upf) { atomicAdd(&hs[s][286 + (upf ? di.up_sym : di.left_sym)], 1u); });
        }
    }
    __syncthreads();
    const size_t b = (size_t)c / PNG_CHUNKS_PER_BLOCK;
    uint32_t* dst = hist + (((size_t)m * B + b) * 2) * PNG_NSYM;
    for (int i = threadIdx.x; i < 2 * PNG_NSYM; i += blockDim.x) {
        const uint32_t v = (&hs[0][0])[i];
        if (v) atomicAdd(dst + i, v);
    }
}

// ---- 5. code tables + block headers ------------------------------------------------------------------------------------------
struct HuffLds {
    uint32_t f[PNG_NSYM];                          // working counts (flattened on a rebuild)
    uint16_t order[PNG_NSYM];                      // nonzero symbols sorted by (count, symbol)
    uint32_t iw[PNG_NSYM];                         // internal node weights, in creation order
    int16_t lpar[PNG_NSYM], ipar[PNG_NSYM];        // parent (internal index) of each sorted leaf / internal node
    uint8_t idep[PNG_NSYM];
    int nz, done;
};

// code lengths (<= maxbits) of freq[0 .. n): the host's huffman_lengths.  Its heap pops the least (weight, node index) and node
// indices are leaves in symbol order, then internal nodes in creation order; merged weights never decrease, so two queues (the
// sorted leaves, the internal nodes as made) pop in the same order: a leaf wins a tie.  One wave; lane 0 does the merge.
__device__ void huffman_lengths(const uint32_t* freq, int n, int maxbits, uint8_t* len, HuffLds* hl) {
    const int lane = threadIdx.x;
    for (int i = lane; i < n; i += 64) hl->f[i] = freq[i];
    __syncthreads();
    for (;;) {
        for (int i = lane; i < n; i += 64) {
            const uint32_t fi = hl->f[i];
            if (!fi) continue;
            int r = 0;
            for (int j = 0; j < n; ++j) {
                const uint32_t fj = hl->f[j];
                r += fj && (fj < fi || (fj == fi && j < i));
            }
            hl->order[r] = (uint16_t)i;
        }
        __syncthreads();
        if (lane == 0) {
            int nz = 0;
            for (int i = 0; i < n; ++i) { nz += hl->f[i] != 0; len[i] = 0; }
            hl->done = 1;
            if (nz == 1) len[hl->order[0]] = 1;
            else if (nz > 1) {
                int li = 0, ii = 0, ni = 0;
                for (int step = 0; step < nz - 1; ++step) {
                    uint32_t wsum = 0;
                    for (int pick = 0; pick < 2; ++pick) {
                        if (li < nz && (ii >= ni || hl->f[hl->order[li]] <= hl->iw[ii])) {
                            wsum += hl->f[hl->order[li]]; hl->lpar[li++] = (int16_t)ni;
                        } else {
                            wsum += hl->iw[ii]; hl->ipar[ii++] = (int16_t)ni;
                        }
                    }
                    hl->iw[ni++] = wsum;
                }
                hl->idep[ni - 1] = 0;
                for (int k = ni - 2; k >= 0; --k) hl->idep[k] = (uint8_t)(hl->idep[hl->ipar[k]] + 1);
                int deepest = 0;
                for (int r = 0; r < nz; ++r) {
                    const int d = hl->idep[hl->lpar[r]] + 1;
                    len[hl->order[r]] = (uint8_t)d;
                    if (d > deepest) deepest = d;
                }
                if (deepest > maxbits) {
                    hl->done = 0;
                    for (int i = 0; i < n; ++i) if (hl->f[i]) hl->f[i] = (hl->f[i] + 1) / 2;
                }
            }
        }
        __syncthreads();
        if (hl->done) break;
    }
}

__device__ void canonical_codes(const uint8_t* len, int n, uint16_t* code) {   // one thread
    int count[16] = {0}, next[16] = {0};
    for (int i = 0; i < n; ++i) count[len[i]]++;
    count[0] = 0;
    int c = 0;
    for (int b = 1; b < 16; ++b) { c = (c + count[b - 1]) << 1; next[b] = c; }
    for (int i = 0; i < n; ++i) {
        if (!len[i]) { code[i] = 0; continue; }
        unsigned v = unsigned(next[len[i]]++), r = 0;
        for (int b = 0; b < len[i]; ++b) { r = (r << 1) | (v & 1); v >>= 1; }
        code[i] = (uint16_t)r;
    }
}

struct BitPut {                                    // LSB-first writer into a zeroed word buffer
    uint32_t* buf;
    uint32_t pos = 0;
    __device__ void put(uint32_t v, int bits) {
        if (!bits) return;
        const uint32_t o = pos & 31, wi = pos >> 5;
        buf[wi] |= v << o;
        if (o + bits > 32) buf[wi + 1] |= v >> (32 - o);
        pos += bits;
    }
};

// grid (B, 2, nm), 64 threads
__global__ __launch_bounds__(64) void png_tables_kernel(const uint32_t* __restrict__ hist, const unsigned long long* __restrict__ meta,
                                                        uint32_t* __restrict__ tables, uint32_t* __restrict__ hdr,
                                                        uint32_t* __restrict__ hdrbits, size_t B) {
    __shared__ HuffLds hl;
    __shared__ uint32_t fl[PNG_NSYM], fc[19];
    __shared__ uint8_t lens[PNG_NSYM], c_len[19];
    __shared__ uint16_t codes[PNG_NSYM], c_code[19], cl[PNG_NSYM];
    __shared__ uint32_t hb[PNG_HDR_WORDS];
    __shared__ int ncl, s_hlit, s_hdist;
    const int b = blockIdx.x, s = blockIdx.y, m = blockIdx.z, lane = threadIdx.x;
    const unsigned long long nblk = meta[(size_t)m * MT_N + MT_NBLK];
    if ((unsigned long long)b >= nblk) return;
    const size_t e = ((size_t)m * B + b) * 2 + s;
    for (int i = lane; i < PNG_NSYM; i += 64) fl[i] = hist[e * PNG_NSYM + i];
    for (int i = lane; i < PNG_HDR_WORDS; i += 64) hb[i] = 0u;
    __syncthreads();
    if (lane == 0) {
        fl[256] = 1;
        bool anyd = false;
        for (int i = 286; i < PNG_NSYM; ++i) anyd |= fl[i] != 0;
        if (!anyd) fl[286] = 1;                    // at least one distance code must be defined
    }
    __syncthreads();
    huffman_lengths(fl, 286, 15, lens, &hl);
    huffman_lengths(fl + 286, 30, 15, lens + 286, &hl);
    if (lane == 0) {
        canonical_codes(lens, 286, codes);
        canonical_codes(lens + 286, 30, codes + 286);
        int hlit = 286, hdist = 30;
        while (hlit > 257 && !lens[hlit - 1]) --hlit;
        while (hdist > 1 && !lens[286 + hdist - 1]) --hdist;
        // the code-length sequence with the 16 / 17 / 18 run symbols: low 5 bits symbol, extra value << 5
        int nc = 0;
        const int total = hlit + hdist;
        auto seq = [&](int i) -> int { return i < hlit ? lens[i] : lens[286 + i - hlit]; };
        for (int i = 0; i < total;) {
            int j = i;
            const int v = seq(i);
            while (j < total && seq(j) == v) ++j;
            int run = j - i;
            if (v == 0) {
                while (run >= 11) { const int r = run > 138 ? 138 : run; cl[nc++] = (uint16_t)(18 | ((r - 11) << 5)); run -= r; }
                if (run >= 3) { cl[nc++] = (uint16_t)(17 | ((run - 3) << 5)); run = 0; }
                while (run--) cl[nc++] = 0;
            } else {
                cl[nc++] = (uint16_t)v; --run;
                while (run >= 3) { const int r = run > 6 ? 6 : run; cl[nc++] = (uint16_t)(16 | ((r - 3) << 5)); run -= r; }
                while (run--) cl[nc++] = (uint16_t)v;
            }
            i = j;
        }
        ncl = nc;
        for (int i = 0; i < 19; ++i) fc[i] = 0;
        for (int i = 0; i < nc; ++i) fc[cl[i] & 31]++;
        s_hlit = hlit; s_hdist = hdist;
    }
    __syncthreads();
    huffman_lengths(fc, 19, 7, c_len, &hl);
    if (lane == 0) {
        canonical_codes(c_len, 19, c_code);
        const int hlit = s_hlit, hdist = s_hdist;
        int hclen = 19;
        while (hclen > 4 && !c_len[kClOrder[hclen - 1]]) --hclen;
        BitPut bw{hb};
        bw.put((unsigned long long)b + 1 == nblk ? 1u : 0u, 1);
        bw.put(2u, 2);
        bw.put((uint32_t)(hlit - 257), 5); bw.put((uint32_t)(hdist - 1), 5); bw.put((uint32_t)(hclen - 4), 4);
        for (int i = 0; i < hclen; ++i) bw.put(c_len[kClOrder[i]], 3);
        for (int i = 0; i < ncl; ++i) {
            const int sym = cl[i] & 31;
            bw.put(c_code[sym], c_len[sym]);
            if (sym == 16) bw.put((uint32_t)(cl[i] >> 5), 2);
            else if (sym == 17) bw.put((uint32_t)(cl[i] >> 5), 3);
            else if (sym == 18) bw.put((uint32_t)(cl[i] >> 5), 7);
        }
        hdrbits[e] = bw.pos;
    }
    __syncthreads();
    for (int i = lane; i < PNG_NSYM; i += 64) tables[e * PNG_NSYM + i] = (uint32_t)codes[i] | ((uint32_t)lens[i] << 16);
    for (int i = lane; i < PNG_HDR_WORDS; i += 64) hdr[e * PNG_HDR_WORDS + i] = hb[i];
}

// ---- token bits --------------------------------------------------------------------------------------------------------------
// emit(v, nbits) for each bit string of token k in stream s under the code table tab (LDS, code | len << 16)
template <class Emit>
__device__ __forceinline__ void token_bits(uint32_t k, int s, const uint32_t* tab, const uint32_t* lut32, const DistInfo& di,
                                           Emit&& emit) {
    token_symbols(k, s, lut32, di,
                  [&](uint32_t sym) { const uint32_t t = tab[sym]; emit(t & 0xffff, (int)(t >> 16)); },
                  [&](int l) {
                      const int c = len_code(l);
                      const uint32_t t = tab[257 + c];
                      const int cl = (int)(t >> 16);
                      emit((t & 0xffff) | ((uint32_t)(l - kLenBase[c]) << cl), cl + kLenExtra[c]);
                  },
                  [&](bool upf) {
                      const int sym = upf ? di.up_sym : di.left_sym;
                      const uint32_t t = tab[286 + sym];
                      const int dl = (int)(t >> 16);
                      const uint32_t ev = upf ? (uint32_t)di.up_eval : 0u;
                      emit((t & 0xffff) | (ev << dl), dl + (upf ? di.up_ebits : 0));
                  });
}

// ---- 6. bits per chunk -------------------------------------------------------------------------------------------------------
// grid (C, nm), 1024 threads
__global__ __launch_bounds__(1024) void png_tokbits_kernel(const uint32_t* __restrict__ tok, const unsigned long long* __restrict__ meta,
                                                           const uint8_t* __restrict__ lut, const uint32_t* __restrict__ tables,
                                                           uint32_t* __restrict__ chunkbits, int w, int up_ok, size_t T, size_t B,
                                                           size_t C) {
    __shared__ uint32_t tab[2][PNG_NSYM];
    __shared__ uint32_t lut32[256];
    __shared__ uint32_t sm[17];
    const int m = blockIdx.y, c = blockIdx.x;
    const unsigned long long* mt = meta + (size_t)m * MT_N;
    if ((unsigned long long)c >= mt[MT_NCHUNK]) return;
    const size_t b = (size_t)c / PNG_CHUNKS_PER_BLOCK;
    for (int i = threadIdx.x; i < 2 * PNG_NSYM; i += blockDim.x) (&tab[0][0])[i] = tables[((size_t)m * B + b) * 2 * PNG_NSYM + i];
    load_lut32(lut, lut32);
    __syncthreads();
    const size_t g = (size_t)c * PNG_CHUNK + threadIdx.x;
    const uint32_t k = g < mt[MT_NTOK] ? tok[(size_t)m * T + g] : 0xffffffffu;
    for (int s = 0; s < 2; ++s) {
        const DistInfo di = dist_info(s, w, up_ok);
        uint32_t nb = 0;
        if (k != 0xffffffffu) token_bits(k, s, tab[s], lut32, di, [&](uint32_t, int bits) { nb += bits; });
        uint32_t tot;
        block_scan_excl(nb, sm, &tot);
        if (threadIdx.x == 0) chunkbits[((size_t)m * 2 + s) * C + c] = tot;
    }
}

// ---- 7. chunk offsets --------------------------------------------------------------------------------------------------------
// grid (2, nm), 1024 threads.  Bit 0 = the first bit after the zlib header.  In front of chunk c = 1024 j (the first chunk of
// deflate block j) sits the end-of-block code of block j - 1 and block j's header: gapoff[j] = where that gap starts;
// gapoff[nblocks] = the final end-of-block code.
__global__ __launch_bounds__(1024) void png_scan_chunks_kernel(const uint32_t* __restrict__ chunkbits, const uint32_t* __restrict__ tables,
                                                               const uint32_t* __restrict__ hdrbits, unsigned long long* __restrict__ meta,
                                                               unsigned long long* __restrict__ chunkoff,
                                                               unsigned long long* __restrict__ gapoff, size_t B, size_t C) {
    __shared__ uint32_t sm[17];
    const int s = blockIdx.x, m = blockIdx.y;
    unsigned long long* mt = meta + (size_t)m * MT_N;
    const size_t nchunk = mt[MT_NCHUNK], nblk = mt[MT_NBLK];
    auto eob_len = [&](size_t b) -> uint32_t { return tables[(((size_t)m * B + b) * 2 + s) * PNG_NSYM + 256] >> 16; };
    unsigned long long carry = 0;
    for (size_t c0 = 0; c0 < nchunk; c0 += 1024) {
        const size_t c = c0 + threadIdx.x;
        uint32_t gap = 0, v = 0;
        if (c < nchunk) {
            if (c % PNG_CHUNKS_PER_BLOCK == 0) {
                const size_t b = c / PNG_CHUNKS_PER_BLOCK;
                gap = (b ? eob_len(b - 1) : 0u) + hdrbits[((size_t)m * B + b) * 2 + s];
            }
            v = gap + chunkbits[((size_t)m * 2 + s) * C + c];
        }
        uint32_t tot;
        const uint32_t ex = block_scan_excl(v, sm, &tot);
        if (c < nchunk) {
            chunkoff[((size_t)m * 2 + s) * C + c] = carry + ex + gap;
            if (c % PNG_CHUNKS_PER_BLOCK == 0) gapoff[((size_t)m * 2 + s) * (B + 1) + c / PNG_CHUNKS_PER_BLOCK] = carry + ex;
        }
        carry += tot;
    }
    if (threadIdx.x == 0) {
        gapoff[((size_t)m * 2 + s) * (B + 1) + nblk] = carry;
        mt[MT_BITS0 + s] = carry + eob_len(nblk - 1);
    }
}

// ---- 8. placement ------------------------------------------------------------------------------------------------------------
__global__ void png_place_kernel(unsigned long long* __restrict__ meta, int nm, long long out_cap, long long* __restrict__ cursor,
                                 long long* __restrict__ table) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long off = (*cursor + 15) & ~15ll;
    for (int m = 0; m < nm; ++m) {
        unsigned long long* mt = meta + (size_t)m * MT_N;
        for (int s = 0; s < 2; ++s) {
            const long long len = png_file_len(mt[MT_BITS0 + s]);
            const bool fits = off + ((len + 15) & ~15ll) <= out_cap;
            table[(m * 2 + s) * 2] = off;
            table[(m * 2 + s) * 2 + 1] = fits ? len : -len - 1;
            mt[MT_OFF0 + s] = fits ? (unsigned long long)off : ~0ull;
            mt[MT_LEN0 + s] = (unsigned long long)len;
            if (fits) off += (len + 15) & ~15ll;
        }
    }
    *cursor = off;
}

// ---- 9. zero the files' ranges -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void png_zero_kernel(const unsigned long long* __restrict__ meta, unsigned char* __restrict__ out) {
    const int s = blockIdx.y, m = blockIdx.z;
    const unsigned long long* mt = meta + (size_t)m * MT_N;
    const unsigned long long off = mt[MT_OFF0 + s];
    if (off == ~0ull) return;
    const size_t n16 = (size_t)((mt[MT_LEN0 + s] + 15) >> 4);
    uint4* p = reinterpret_cast<uint4*>(out + off);
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// ---- 10. pack ----------------------------------------------------------------------------------------------------------------
// grid (C, 2, nm), 1024 threads.  `out` is 16-byte aligned and the file offsets are multiples of 16, so bit positions relative to
// `out` have the alignment of absolute ones.
__global__ __launch_bounds__(1024) void png_pack_kernel(const uint32_t* __restrict__ tok, const unsigned long long* __restrict__ meta,
                                                        const uint8_t* __restrict__ lut, const uint32_t* __restrict__ tables,
                                                        const unsigned long long* __restrict__ chunkoff, const uint32_t* __restrict__ chunkbits,
                                                        unsigned char* __restrict__ out, int w, int up_ok, size_t T, size_t B, size_t C) {
    __shared__ uint32_t tab[PNG_NSYM];
    __shared__ uint32_t lut32[256];
    __shared__ uint32_t sm[17];
    __shared__ uint32_t buf[PNG_PACK_WORDS];
    const int c = blockIdx.x, s = blockIdx.y, m = blockIdx.z;
    const unsigned long long* mt = meta + (size_t)m * MT_N;
    if ((unsigned long long)c >= mt[MT_NCHUNK] || mt[MT_OFF0 + s] == ~0ull) return;
    const size_t b = (size_t)c / PNG_CHUNKS_PER_BLOCK;
    for (int i = threadIdx.x; i < PNG_NSYM; i += blockDim.x) tab[i] = tables[(((size_t)m * B + b) * 2 + s) * PNG_NSYM + i];
    load_lut32(lut, lut32);
    for (int i = threadIdx.x; i < PNG_PACK_WORDS; i += blockDim.x) buf[i] = 0u;
    __syncthreads();
    const DistInfo di = dist_info(s, w, up_ok);
    const size_t g = (size_t)c * PNG_CHUNK + threadIdx.x;
    const uint32_t k = g < mt[MT_NTOK] ? tok[(size_t)m * T + g] : 0xffffffffu;
    uint32_t nb = 0;
    if (k != 0xffffffffu) token_bits(k, s, tab, lut32, di, [&](uint32_t, int bits) { nb += bits; });
    uint32_t tot;
    const uint32_t my = block_scan_excl(nb, sm, &tot);
    const unsigned long long bit0 = (mt[MT_OFF0 + s] + 43) * 8 + chunkoff[((size_t)m * 2 + s) * C + c];
    const unsigned long long w0 = bit0 >> 5;
    const uint32_t lead = (uint32_t)(bit0 & 31);
    if (k != 0xffffffffu) {
        uint32_t pos = lead + my;
        token_bits(k, s, tab, lut32, di, [&](uint32_t v, int bits) {
            if (!bits) return;
            const uint32_t o = pos & 31, wi = pos >> 5;
            atomicOr(&buf[wi], v << o);
            if (o + bits > 32) atomicOr(&buf[wi + 1], v >> (32 - o));
            pos += bits;
        });
    }
    __syncthreads();
    if (!tot) return;
    const uint32_t nw = (lead + tot + 31) >> 5;
    uint32_t* dst = reinterpret_cast<uint32_t*>(out) + w0;
    for (uint32_t i = threadIdx.x; i < nw; i += blockDim.x) {
        if (i == 0 || i == nw - 1) atomicOr(dst + i, buf[i]);        // shared with the neighbouring chunk / header
        else dst[i] = buf[i];
    }
}

// ---- 11. block headers + end-of-block codes ----------------------------------------------------------------------------------
// grid (B + 1, 2, nm), 64 threads
__global__ __launch_bounds__(64) void png_headers_kernel(const unsigned long long* __restrict__ meta, const uint32_t* __restrict__ tables,
                                                         const uint32_t* __restrict__ hdr, const uint32_t* __restrict__ hdrbits,
                                                         const unsigned long long* __restrict__ gapoff, unsigned char* __restrict__ out,
                                                         size_t B) {
    const int b = blockIdx.x, s = blockIdx.y, m = blockIdx.z;
    const unsigned long long* mt = meta + (size_t)m * MT_N;
    const unsigned long long nblk = mt[MT_NBLK];
    if ((unsigned long long)b > nblk || mt[MT_OFF0 + s] == ~0ull) return;
    uint32_t* o32 = reinterpret_cast<uint32_t*>(out);
    unsigned long long pos = (mt[MT_OFF0 + s] + 43) * 8 + gapoff[((size_t)m * 2 + s) * (B + 1) + b];
    auto orbits = [&](unsigned long long at, uint32_t v, uint32_t bits) {
        const uint32_t sh = (uint32_t)(at & 31);
        uint32_t* p = o32 + (at >> 5);
        if (v << sh) atomicOr(p, v << sh);
        if (sh && sh + bits > 32 && (v >> (32 - sh))) atomicOr(p + 1, v >> (32 - sh));
    };
    if (b > 0) {
        const uint32_t t = tables[(((size_t)m * B + b - 1) * 2 + s) * PNG_NSYM + 256];
        if (threadIdx.x == 0) orbits(pos, t & 0xffff, t >> 16);
        pos += t >> 16;
    }
    if ((unsigned long long)b == nblk) return;
    const size_t e = ((size_t)m * B + b) * 2 + s;
    const uint32_t nbits = hdrbits[e];
    for (uint32_t i = threadIdx.x; i * 32 < nbits; i += 64) {
        const uint32_t bits = nbits - i * 32 < 32 ? nbits - i * 32 : 32;
        orbits(pos + 32ull * i, hdr[e * PNG_HDR_WORDS + i], bits);
    }
}

// ---- 12. Adler-32 per row ----------------------------------------------------------------------------------------------------
// Adler-32 of N bytes d_0 .. d_{N-1}: A = 1 + sum d_i, B = N + sum (N - i) d_i (mod 65521).  Row r (L bytes from p = r L) adds
// S_r = sum d_j and (N - p - L) S_r + U_r with U_r = sum_j (L - j) d_j.  grid (h, 2, nm), 64 threads
__global__ __launch_bounds__(64) void png_adler_rows_kernel(const uint8_t* __restrict__ maps, const uint8_t* __restrict__ lut,
                                                            const unsigned long long* __restrict__ meta, uint32_t* __restrict__ adler,
                                                            int h, int w) {
    __shared__ unsigned long long sS[64], sU[64];
    const int y = blockIdx.x, s = blockIdx.y, m = blockIdx.z, lane = threadIdx.x;
    if (meta[(size_t)m * MT_N + MT_OFF0 + s] == ~0ull) return;
    const uint8_t* g = maps + ((size_t)m * h + y) * w;
    const unsigned long long L = (unsigned long long)w * (s ? 3 : 1) + 1;
    unsigned long long S = 0, U = 0;
    for (int x = lane; x < w; x += 64) {
        const uint32_t v = g[x];
        if (s == 0) { S += v; U += (L - 1 - x) * v; }
        else {
            const unsigned long long j = 1 + 3ull * x;
            const uint32_t c0 = lut[3 * v], c1 = lut[3 * v + 1], c2 = lut[3 * v + 2];
            S += c0 + c1 + c2;
            U += (L - j) * c0 + (L - j - 1) * c1 + (L - j - 2) * c2;
        }
    }
    sS[lane] = S; sU[lane] = U;
    __syncthreads();
    if (lane == 0) {
        unsigned long long a = 0, u = 0;
        for (int i = 0; i < 64; ++i) { a += sS[i]; u += sU[i]; }
        uint32_t* d = adler + (((size_t)m * 2 + s) * h + y) * 2;
        d[0] = (uint32_t)(a % PNG_ADLER_MOD);
        d[1] = (uint32_t)(u % PNG_ADLER_MOD);
    }
}

// ---- 13. Adler-32 + framing --------------------------------------------------------------------------------------------------
// grid (2, nm), 64 threads
__global__ __launch_bounds__(64) void png_frame_kernel(const unsigned long long* __restrict__ meta, const uint32_t* __restrict__ adler,
                                                       unsigned char* __restrict__ out, int h, int w) {
    __shared__ unsigned long long sA[64], sB[64];
    const int s = blockIdx.x, m = blockIdx.y, lane = threadIdx.x;
    const unsigned long long* mt = meta + (size_t)m * MT_N;
    const unsigned long long off = mt[MT_OFF0 + s];
    if (off == ~0ull) return;
    const unsigned long long L = (unsigned long long)w * (s ? 3 : 1) + 1;
    const unsigned long long Lm = L % PNG_ADLER_MOD;
    unsigned long long A = 0, Bs = 0;
    for (int y = lane; y < h; y += 64) {
        const uint32_t* d = adler + (((size_t)m * 2 + s) * h + y) * 2;
        const unsigned long long S = d[0], U = d[1];
        const unsigned long long after = ((unsigned long long)(h - 1 - y) % PNG_ADLER_MOD) * Lm % PNG_ADLER_MOD;
        A += S;
        Bs += (after * S + U) % PNG_ADLER_MOD;
    }
    sA[lane] = A; sB[lane] = Bs;
    __syncthreads();
    if (lane != 0) return;
    for (int i = 1; i < 64; ++i) { A += sA[i]; Bs += sB[i]; }
    const unsigned long long N = (unsigned long long)h * L;
    const uint32_t a32 = (uint32_t)((1 + A) % PNG_ADLER_MOD);
    const uint32_t b32 = (uint32_t)((N % PNG_ADLER_MOD + Bs) % PNG_ADLER_MOD);
    unsigned char* f = out + off;
    const unsigned char sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    for (int i = 0; i < 8; ++i) f[i] = sig[i];
    put_be32(f + 8, 13u);
    f[12] = 'I'; f[13] = 'H'; f[14] = 'D'; f[15] = 'R';
    put_be32(f + 16, (uint32_t)w);
    put_be32(f + 20, (uint32_t)h);
    f[24] = 8; f[25] = s ? 2 : 0; f[26] = 0; f[27] = 0; f[28] = 0;
    put_be32(f + 29, crc_bytes_slow(0u, f + 12, 17));
    const unsigned long long bytes = (mt[MT_BITS0 + s] + 7) >> 3;
    put_be32(f + 33, (uint32_t)(2 + bytes + 4));
    f[37] = 'I'; f[38] = 'D'; f[39] = 'A'; f[40] = 'T';
    f[41] = 0x78; f[42] = 0x9c;
    unsigned char* e = f + 43 + bytes;
    put_be32(e, (b32 << 16) | a32);
    // e + 4: the IDAT CRC (png_crc_finish_kernel); then IEND
    put_be32(e + 8, 0u);
    e[12] = 'I'; e[13] = 'E'; e[14] = 'N'; e[15] = 'D';
    put_be32(e + 16, 0xae426082u);
}

// ---- 14. IDAT CRC pieces -----------------------------------------------------------------------------------------------------
// CRC register update is linear: reg(I, D) = I x^(8|D|) + reg(0, D) (mod P), and reg(0, D) = sum over pieces of reg(0, piece)
// x^(8 * bytes after the piece).  grid (P, 2, nm), 256 threads; the sums are XORs (order-free)
__global__ __launch_bounds__(256) void png_crc_kernel(unsigned long long* __restrict__ meta, const unsigned char* __restrict__ out) {
    __shared__ uint32_t tbl[256];
    __shared__ uint32_t red[4];
    const int s = blockIdx.y, m = blockIdx.z;
    const unsigned long long* mt = meta + (size_t)m * MT_N;
    const unsigned long long off = mt[MT_OFF0 + s];
    if (off == ~0ull) return;
    const unsigned long long D = 4 + 2 + ((mt[MT_BITS0 + s] + 7) >> 3) + 4;     // "IDAT" + zlib stream
    const unsigned long long p0 = ((unsigned long long)blockIdx.x * 256) * PNG_CRC_PIECE;
    if (p0 >= D) return;
    {
        uint32_t c = threadIdx.x;
        for (int k = 0; k < 8; ++k) c = c & 1 ? (c >> 1) ^ 0xedb88320u : c >> 1;
        tbl[threadIdx.x] = c;
    }
    __syncthreads();
    const unsigned long long a = p0 + (unsigned long long)threadIdx.x * PNG_CRC_PIECE;
    uint32_t r = 0;
    if (a < D) {
        const unsigned long long e = a + PNG_CRC_PIECE < D ? a + PNG_CRC_PIECE : D;
        const unsigned char* d = out + off + 37;
        uint32_t c = 0;
        for (unsigned long long i = a; i < e; ++i) c = tbl[(c ^ d[i]) & 0xff] ^ (c >> 8);
        r = c ? crc_mult(crc_x8n(D - e), c) : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) r ^= __shfl_xor(r, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t v = red[0] ^ red[1] ^ red[2] ^ red[3];
        if (v) atomicXor(reinterpret_cast<uint32_t*>(meta + (size_t)m * MT_N + MT_CRC0 + s), v);   // low half (little-endian)
    }
}

// ---- 15. IDAT CRC ------------------------------------------------------------------------------------------------------------
__global__ void png_crc_finish_kernel(const unsigned long long* __restrict__ meta, unsigned char* __restrict__ out, int nm) {
    const int i = threadIdx.x;
    if (i >= 2 * nm) return;
    const int m = i >> 1, s = i & 1;
    const unsigned long long* mt = meta + (size_t)m * MT_N;
    const unsigned long long off = mt[MT_OFF0 + s];
    if (off == ~0ull) return;
    const unsigned long long bytes = (mt[MT_BITS0 + s] + 7) >> 3;
    const unsigned long long D = 4 + 2 + bytes + 4;
    const uint32_t acc = (uint32_t)mt[MT_CRC0 + s];
    const uint32_t crc = crc_mult(crc_x8n(D), 0xffffffffu) ^ acc ^ 0xffffffffu;
    put_be32(out + off + 43 + bytes + 4, crc);
}

}  // namespace

size_t png_scratch_bytes(int n, int h, int w) {
    const int nm = n < PNG_MAPS ? n : PNG_MAPS;
    size_t bytes = 0;
    carve(nullptr, nm, h, w, &bytes);
    return bytes;
}

size_t png_worst_file_bytes(int h, int w) {
    const size_t T = (size_t)h * (w + 1), B = (T + (1u << PNG_BLOCK_SHIFT) - 1) >> PNG_BLOCK_SHIFT;
    // colour: <= 45 bits per pixel (three 15-bit literals), 15 per filter byte; per block <= 4498 header + 15 end-of-block bits
    const size_t bits = (size_t)h * w * 45 + (size_t)h * 15 + B * 4513;
    return 63 + (bits + 7) / 8;
}

// ---- the stages that do not look at tokens, for `streams` streams of each of nm files' slots (kernels.h) -----------------------
void png_stage_tables(const PngStageBuffers& L, int nm, int streams, hipStream_t st) {
    png_tables_kernel<<<dim3((unsigned)L.B, streams, nm), 64, 0, st>>>(L.hist, L.meta, L.tables, L.hdr, L.hdrbits, L.B);
}
void png_stage_offsets(const PngStageBuffers& L, int nm, int streams, hipStream_t st) {
    png_scan_chunks_kernel<<<dim3(streams, nm), 1024, 0, st>>>(L.chunkbits, L.tables, L.hdrbits, L.meta, L.chunkoff, L.gapoff, L.B, L.C);
}
void png_stage_zero(const PngStageBuffers& L, unsigned char* out, int nm, int streams, hipStream_t st) {
    png_zero_kernel<<<dim3(256, streams, nm), 256, 0, st>>>(L.meta, out);
}
void png_stage_headers(const PngStageBuffers& L, unsigned char* out, int nm, int streams, hipStream_t st) {
    png_headers_kernel<<<dim3((unsigned)L.B + 1, streams, nm), 64, 0, st>>>(L.meta, L.tables, L.hdr, L.hdrbits, L.gapoff, out, L.B);
}
void png_stage_crc(const PngStageBuffers& L, unsigned char* out, int nm, int streams, size_t worst_file_bytes, hipStream_t st) {
    const unsigned crc_blocks = (unsigned)((worst_file_bytes + 256ull * PNG_CRC_PIECE - 1) / (256ull * PNG_CRC_PIECE));
    png_crc_kernel<<<dim3(crc_blocks, streams, nm), 256, 0, st>>>(L.meta, out);
    png_crc_finish_kernel<<<1, 64, 0, st>>>(L.meta, out, nm);
}

hipError_t launch_png_encode(const uint8_t* maps, int n, int h, int w, const uint8_t* lut, void* scratch, unsigned char* out,
                             long long out_cap, long long* cursor, long long* table, hipStream_t st) {
    if (n < 1 || h < 1 || w < 1 || h > 65536 || w > 65536 || ((size_t)3 * w + 1) * h > 0x7fffffffull) return hipErrorInvalidValue;
    const int up_ok = (size_t)w * 3 + 1 <= 32768 ? 1 : 0;
    const size_t worst = png_worst_file_bytes(h, w);
    for (int p0 = 0; p0 < n; p0 += PNG_MAPS) {
        const int nm = n - p0 < PNG_MAPS ? n - p0 : PNG_MAPS;
        const Layout L = carve(scratch, nm, h, w, nullptr);
        const uint8_t* mp = maps + (size_t)p0 * h * w;
        long long* tb = table + (size_t)p0 * 4;
        hipError_t err;
        if ((err = hipMemsetAsync(L.meta, 0, (size_t)nm * MT_N * 8, st)) != hipSuccess) return err;
        if ((err = hipMemsetAsync(L.hist, 0, (size_t)nm * L.B * 2 * PNG_NSYM * 4, st)) != hipSuccess) return err;
        const unsigned C = (unsigned)L.C;
        const PngStageBuffers S{L.meta, L.hist, L.tables, L.hdr, L.hdrbits, L.chunkbits, L.chunkoff, L.gapoff, L.B, L.C};
        png_parse_kernel<<<dim3((h + 63) / 64, nm), 64, 0, st>>>(mp, L.slot, L.rowcnt, h, w, up_ok, L.T);
        png_scan_rows_kernel<<<nm, 1024, 0, st>>>(L.rowcnt, L.rowoff, L.meta, h);
        png_compact_kernel<<<dim3(h, nm), 256, 0, st>>>(L.slot, L.rowcnt, L.rowoff, L.tok, h, w, L.T);
        png_hist_kernel<<<dim3(C, nm), PNG_CHUNK, 0, st>>>(L.tok, L.meta, lut, L.hist, w, up_ok, L.T, L.B);
        png_stage_tables(S, nm, 2, st);
        png_tokbits_kernel<<<dim3(C, nm), PNG_CHUNK, 0, st>>>(L.tok, L.meta, lut, L.tables, L.chunkbits, w, up_ok, L.T, L.B, L.C);
        png_stage_offsets(S, nm, 2, st);
        png_place_kernel<<<1, 64, 0, st>>>(L.meta, nm, out_cap, cursor, tb);
        png_stage_zero(S, out, nm, 2, st);
        png_pack_kernel<<<dim3(C, 2, nm), PNG_CHUNK, 0, st>>>(L.tok, L.meta, lut, L.tables, L.chunkoff, L.chunkbits, out, w, up_ok,
                                                              L.T, L.B, L.C);
        png_stage_headers(S, out, nm, 2, st);
        png_adler_rows_kernel<<<dim3(h, 2, nm), 64, 0, st>>>(mp, lut, L.meta, L.adler, h, w);
        png_frame_kernel<<<dim3(2, nm), 64, 0, st>>>(L.meta, L.adler, out, h, w);
        png_stage_crc(S, out, nm, 2, worst, st);
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    return hipSuccess;
}
