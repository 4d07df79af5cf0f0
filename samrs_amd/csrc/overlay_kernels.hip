// overlay_kernels.hip -- visualize.py's overlays on the device (gfx950): the blend of an image with its painted class map, and a
// truecolour PNG encoder for arbitrary uint8 RGB pixels (the blend's output, or anything else).
//
// Blend: out = Image.blend(image, lut[map], alpha) as Pillow computes it, per byte (uint8)((int)a + alpha * ((int)b - (int)a)) in
// float: the product rounded, the sum rounded, the result truncated (__fmul_rn / __fadd_rn, so the compiler cannot contract them).
// The batch is one flat run of pixels: 16 pixels per thread (one 16-byte load of labels, three of image bytes, three stores)
// where the three pointers are 16-byte aligned, a scalar tail (or everything, for unaligned pointers) behind them.
//
// Encoder: 8-bit colour type 2, not interlaced, one IDAT, zlib header 78 9c.  The deflate stream holds the filtered bytes as
// literals only: one dynamic-Huffman block per 2^20 filtered bytes (PNG_BLOCK_SHIFT, the label encoder's block of 2^20 tokens), no
// LZ77 matches.  A symbol here is one filtered byte, so the label encoder's scratch layout and every stage of it that does not look
// at tokens serve as they are (png_stage_* in kernels.h run png_kernels.hip's own kernels for stream 0 of each file's slot).
// Per pass of up to PNG_MAPS images:
//   1. rgb_filter_kernel     block = row: the row's filter (forced, or the least sum of |filtered byte as int8| with ties to the lowest
//                            number), the filtered row = filter byte + 3 w bytes, and the row's Adler sums of those bytes
//   2. rgb_hist_kernel       block = 1024 bytes (a chunk): literal histogram, LDS atomics, then integer atomics into the block's
//   3. png_tables_kernel     (png_kernels.hip) Huffman lengths with the length limit, canonical codes, the block header's bits
//   4. rgb_chunkbits_kernel  block = chunk: code lengths of its bytes -> the chunk's bit count
//   5. png_scan_chunks_kernel (png_kernels.hip) chunk bit offsets, header / end-of-block gaps, the stream's bit count
//   6. rgb_place_kernel      one thread: file lengths -> 16-byte aligned offsets behind *cursor, (offset, length) table, cursor
//   7. png_zero_kernel       (png_kernels.hip) the files' byte ranges are zeroed
//   8. rgb_pack_kernel       block = chunk: the chunk's codes assembled in LDS, whole words stored, the two edge words OR-ed
//   9. png_headers_kernel    (png_kernels.hip) end-of-block codes + block headers, OR-ed
//  10. rgb_frame_kernel      wave = file: Adler-32 = combination of the row sums; signature, IHDR, IDAT head, zlib header, Adler, IEND
//  11. png_crc_kernel, png_crc_finish_kernel (png_kernels.hip) the IDAT CRC by GF(2) shifts.
// Integer work only; every cross-block dependence is a kernel boundary, nothing spins on global memory, and every atomic is an
// order-free integer sum / OR / XOR: the bytes of a file are a function of its pixels and `filter`.
#include "common.h"
#include "kernels.h"
#include "png_device.h"
#include "../../include/samrs_hip.h"

static_assert(SAMRS_PNG_RGB_BLOCK_BYTES == 1 << PNG_BLOCK_SHIFT, "the public header states the deflate block size");

namespace {

// ---- blend -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t blend_byte(uint32_t a, uint32_t b, float alpha) {
    const float d = (float)((int)b - (int)a);
    return (uint32_t)(int)__fadd_rn((float)(int)a, __fmul_rn(alpha, d)) & 0xffu;
}

constexpr int BLEND_PX = 16;                     // pixels per thread of the wide path

// nvec groups of 16 pixels through 16-byte accesses, then pixels [16 nvec, total) one by one; grid-stride over both
__global__ __launch_bounds__(256) void blend_labels_kernel(const uint8_t* __restrict__ images, const uint8_t* __restrict__ maps,
                                                           const uint8_t* __restrict__ lut, float alpha, uint8_t* __restrict__ out,
                                                           size_t nvec, size_t total) {
    __shared__ uint32_t lut32[256];
    for (int i = threadIdx.x; i < 256; i += blockDim.x)
        lut32[i] = (uint32_t)lut[3 * i] | ((uint32_t)lut[3 * i + 1] << 8) | ((uint32_t)lut[3 * i + 2] << 16);
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (size_t g = t0; g < nvec; g += stride) {
        const uint4 mv = reinterpret_cast<const uint4*>(maps)[g];
        const uint4* ip = reinterpret_cast<const uint4*>(images) + 3 * g;
        const uint4 i0 = ip[0], i1 = ip[1], i2 = ip[2];
        const uint32_t mw[4] = {mv.x, mv.y, mv.z, mv.w};
        const uint32_t iw[12] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w, i2.x, i2.y, i2.z, i2.w};
        uint32_t ow[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) ow[k] = 0u;
#pragma unroll
        for (int k = 0; k < 3 * BLEND_PX; ++k) {
            const int px = k / 3, ch = k % 3;
            const uint32_t a = (iw[k >> 2] >> (8 * (k & 3))) & 0xffu;
            const uint32_t lab = (mw[px >> 2] >> (8 * (px & 3))) & 0xffu;
            const uint32_t b = (lut32[lab] >> (8 * ch)) & 0xffu;
            ow[k >> 2] |= blend_byte(a, b, alpha) << (8 * (k & 3));
        }
        uint4* op = reinterpret_cast<uint4*>(out) + 3 * g;
        op[0] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        op[1] = make_uint4(ow[4], ow[5], ow[6], ow[7]);
        op[2] = make_uint4(ow[8], ow[9], ow[10], ow[11]);
    }
    for (size_t p = nvec * BLEND_PX + t0; p < total; p += stride) {
        const uint32_t c = lut32[maps[p]];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[3 * p + ch] = (uint8_t)blend_byte(images[3 * p + ch], (c >> (8 * ch)) & 0xffu, alpha);
    }
}

// ---- truecolour encoder ------------------------------------------------------------------------------------------------------
constexpr int RGB_PACK_WORDS = (PNG_CHUNK * 15 + 31) / 32 + 2;      // a literal's code has at most 15 bits

struct RgbLayout {                                // scratch of one pass; S: the part the label encoder's stages work on
    PngStageBuffers S;
    uint32_t* adler;                              // [nm][h][2] row sums
    uint8_t* filt;                                // [nm][stride] filtered bytes
    size_t N, stride;                             // filtered bytes per image, and their 256-byte aligned pitch
};

RgbLayout rgb_carve(void* base, int nm, int h, int w, size_t* bytes) {
    RgbLayout L;
    L.N = ((size_t)3 * w + 1) * h;
    L.stride = align256(L.N);
    const size_t C = (L.N + PNG_CHUNK - 1) / PNG_CHUNK, B = (L.N + (1u << PNG_BLOCK_SHIFT) - 1) >> PNG_BLOCK_SHIFT;
    L.S.B = B; L.S.C = C;
    unsigned char* p = static_cast<unsigned char*>(base);
    size_t used = 0;
    auto take = [&](size_t n) { unsigned char* q = p ? p + used : nullptr; used += align256(n); return q; };
    L.S.meta = reinterpret_cast<unsigned long long*>(take((size_t)nm * MT_N * 8));
    L.S.hist = reinterpret_cast<uint32_t*>(take((size_t)nm * B * 2 * PNG_NSYM * 4));
    L.S.tables = reinterpret_cast<uint32_t*>(take((size_t)nm * B * 2 * PNG_NSYM * 4));
    L.S.hdr = reinterpret_cast<uint32_t*>(take((size_t)nm * B * 2 * PNG_HDR_WORDS * 4));
    L.S.hdrbits = reinterpret_cast<uint32_t*>(take((size_t)nm * B * 2 * 4));
    L.S.chunkbits = reinterpret_cast<uint32_t*>(take((size_t)nm * 2 * C * 4));
    L.S.chunkoff = reinterpret_cast<unsigned long long*>(take((size_t)nm * 2 * C * 8));
    L.S.gapoff = reinterpret_cast<unsigned long long*>(take((size_t)nm * 2 * (B + 1) * 8));
    L.adler = reinterpret_cast<uint32_t*>(take((size_t)nm * h * 8));
    L.filt = reinterpret_cast<uint8_t*>(take((size_t)nm * L.stride));
    if (bytes) *bytes = used;
    return L;
}

// ---- 1. filter ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
// PNG filter ft of byte x with a = the byte 3 to the left, b = the byte above, c = the byte above a (0 outside the image)
__device__ __forceinline__ uint32_t filter_byte(int ft, int x, int a, int b, int c) {
    switch (ft) {
        case 0: return (uint32_t)x;
        case 1: return (uint32_t)(x - a) & 0xffu;
        case 2: return (uint32_t)(x - b) & 0xffu;
        case 3: return (uint32_t)(x - ((a + b) >> 1)) & 0xffu;
        default: return (uint32_t)(x - paeth(a, b, c)) & 0xffu;
    }
}

// sum over the block's 256 threads (4 waves) into every thread; red: [4]
template <class T>
__device__ __forceinline__ T block_sum256(T v, T* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// grid (h, nm), 256 threads.  filter 0 .. 4: that filter; < 0: per row the filter with the least sum of the filtered bytes taken as
// int8 magnitudes (v < 128 ? v : 256 - v), the lowest number on a tie.  Block (0, m) also writes the image's counts into meta.
__global__ __launch_bounds__(256) void rgb_filter_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ filt,
                                                         uint32_t* __restrict__ adler, unsigned long long* __restrict__ meta, int h,
                                                         int w, int filter, size_t N, size_t stride) {
    __shared__ uint32_t red32[4];
    __shared__ unsigned long long red64[4];
    const int y = blockIdx.x, m = blockIdx.y, rb = 3 * w;
    const uint8_t* row = rgb + ((size_t)m * h + y) * rb;
    const uint8_t* up = y > 0 ? row - rb : nullptr;
    if (y == 0 && threadIdx.x == 0) {
        unsigned long long* mt = meta + (size_t)m * MT_N;
        mt[MT_NTOK] = N;
        mt[MT_NBLK] = (N + (1u << PNG_BLOCK_SHIFT) - 1) >> PNG_BLOCK_SHIFT;
        mt[MT_NCHUNK] = (N + PNG_CHUNK - 1) / PNG_CHUNK;
    }
    int ft = filter;
    if (ft < 0) {
        uint32_t sum[5] = {0u, 0u, 0u, 0u, 0u};
        for (int i = threadIdx.x; i < rb; i += 256) {
            const int x = row[i], a = i >= 3 ? row[i - 3] : 0, b = up ? up[i] : 0, c = (up && i >= 3) ? up[i - 3] : 0;
#pragma unroll
            for (int f = 0; f < 5; ++f) {
                const uint32_t v = filter_byte(f, x, a, b, c);
                sum[f] += v < 128u ? v : 256u - v;
            }
        }
        uint32_t best = 0;
        ft = 0;
#pragma unroll
        for (int f = 0; f < 5; ++f) {
            const uint32_t tot = block_sum256(sum[f], red32);
            if (f == 0 || tot < best) { best = tot; ft = f; }       // strict: a tie keeps the lower number
        }
    }
    const unsigned long long L = (unsigned long long)rb + 1;
    uint8_t* dst = filt + (size_t)m * stride + (size_t)y * L;
    unsigned long long S = 0, U = 0;
    for (int i = threadIdx.x; i < rb; i += 256) {
        const int x = row[i], a = i >= 3 ? row[i - 3] : 0, b = up ? up[i] : 0, c = (up && i >= 3) ? up[i - 3] : 0;
        const uint32_t v = filter_byte(ft, x, a, b, c);
        dst[1 + i] = (uint8_t)v;
        S += v;
        U += (L - 1 - (unsigned long long)i) * v;
    }
    S = block_sum256(S, red64);
    U = block_sum256(U, red64);
    if (threadIdx.x == 0) {
        dst[0] = (uint8_t)ft;
        uint32_t* d = adler + ((size_t)m * h + y) * 2;
        d[0] = (uint32_t)((S + (unsigned long long)ft) % PNG_ADLER_MOD);
        d[1] = (uint32_t)((U + L * (unsigned long long)ft) % PNG_ADLER_MOD);
    }
}

// ---- 2. histograms -----------------------------------------------------------------------------------------------------------
// grid (C, nm), 1024 threads; stream 0 of the slot (m, b)
__global__ __launch_bounds__(1024) void rgb_hist_kernel(const uint8_t* __restrict__ filt, uint32_t* __restrict__ hist, size_t N,
                                                        size_t stride, size_t B) {
    __shared__ uint32_t hs[256];
    const int m = blockIdx.y, c = blockIdx.x;
    if (threadIdx.x < 256) hs[threadIdx.x] = 0u;
    __syncthreads();
    const size_t g = (size_t)c * PNG_CHUNK + threadIdx.x;
    if (g < N) atomicAdd(&hs[filt[(size_t)m * stride + g]], 1u);
    __syncthreads();
    const size_t b = (size_t)c / PNG_CHUNKS_PER_BLOCK;
    uint32_t* dst = hist + (((size_t)m * B + b) * 2) * PNG_NSYM;
    if (threadIdx.x < 256) {
        const uint32_t v = hs[threadIdx.x];
        if (v) atomicAdd(dst + threadIdx.x, v);
    }
}

// ---- 4. bits per chunk -------------------------------------------------------------------------------------------------------
// grid (C, nm), 1024 threads
__global__ __launch_bounds__(1024) void rgb_chunkbits_kernel(const uint8_t* __restrict__ filt, const uint32_t* __restrict__ tables,
                                                             uint32_t* __restrict__ chunkbits, size_t N, size_t stride, size_t B,
                                                             size_t C) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t sm[17];
    const int m = blockIdx.y, c = blockIdx.x;
    const size_t b = (size_t)c / PNG_CHUNKS_PER_BLOCK;
    if (threadIdx.x < 256) tab[threadIdx.x] = tables[(((size_t)m * B + b) * 2) * PNG_NSYM + threadIdx.x];
    __syncthreads();
    const size_t g = (size_t)c * PNG_CHUNK + threadIdx.x;
    const uint32_t nb = g < N ? tab[filt[(size_t)m * stride + g]] >> 16 : 0u;
    uint32_t tot;
    block_scan_excl(nb, sm, &tot);
    if (threadIdx.x == 0) chunkbits[((size_t)m * 2) * C + c] = tot;
}

// ---- 6. placement ------------------------------------------------------------------------------------------------------------
// one file per image; stream 1 of every slot is marked absent for the CRC stage
__global__ void rgb_place_kernel(unsigned long long* __restrict__ meta, int nm, long long out_cap, long long* __restrict__ cursor,
                                 long long* __restrict__ table) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    long long off = (*cursor + 15) & ~15ll;
    for (int m = 0; m < nm; ++m) {
        unsigned long long* mt = meta + (size_t)m * MT_N;
        const long long len = png_file_len(mt[MT_BITS0]);
        const bool fits = off + ((len + 15) & ~15ll) <= out_cap;
        table[m * 2] = off;
        table[m * 2 + 1] = fits ? len : -len - 1;
        mt[MT_OFF0] = fits ? (unsigned long long)off : ~0ull;
        mt[MT_LEN0] = (unsigned long long)len;
        mt[MT_OFF1] = ~0ull;
        if (fits) off += (len + 15) & ~15ll;
    }
    *cursor = off;
}

// ---- 8. pack -----------------------------------------------------------------------------------------------------------------
// grid (C, nm), 1024 threads.  `out` is 16-byte aligned and the file offsets are multiples of 16, so bit positions relative to
// `out` have the alignment of absolute ones.
__global__ __launch_bounds__(1024) void rgb_pack_kernel(const uint8_t* __restrict__ filt, const unsigned long long* __restrict__ meta,
                                                        const uint32_t* __restrict__ tables,
                                                        const unsigned long long* __restrict__ chunkoff,
                                                        unsigned char* __restrict__ out, size_t N, size_t stride, size_t B, size_t C) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t sm[17];
    __shared__ uint32_t buf[RGB_PACK_WORDS];
    const int c = blockIdx.x, m = blockIdx.y;
    const unsigned long long* mt = meta + (size_t)m * MT_N;
    if (mt[MT_OFF0] == ~0ull) return;
    const size_t b = (size_t)c / PNG_CHUNKS_PER_BLOCK;
    if (threadIdx.x < 256) tab[threadIdx.x] = tables[(((size_t)m * B + b) * 2) * PNG_NSYM + threadIdx.x];
    for (int i = threadIdx.x; i < RGB_PACK_WORDS; i += blockDim.x) buf[i] = 0u;
    __syncthreads();
    const size_t g = (size_t)c * PNG_CHUNK + threadIdx.x;
    const uint32_t t = g < N ? tab[filt[(size_t)m * stride + g]] : 0u;
    const uint32_t bits = t >> 16, code = t & 0xffffu;
    uint32_t tot;
    const uint32_t my = block_scan_excl(bits, sm, &tot);
    const unsigned long long bit0 = (mt[MT_OFF0] + 43) * 8 + chunkoff[((size_t)m * 2) * C + c];
    const unsigned long long w0 = bit0 >> 5;
    const uint32_t lead = (uint32_t)(bit0 & 31);
    if (bits) {
        const uint32_t pos = lead + my, o = pos & 31, wi = pos >> 5;
        atomicOr(&buf[wi], code << o);
        if (o + bits > 32) atomicOr(&buf[wi + 1], code >> (32 - o));
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

// ---- 10. Adler-32 + framing --------------------------------------------------------------------------------------------------
// Adler-32 of N bytes d_0 .. d_{N-1}: A = 1 + sum d_i, B = N + sum (N - i) d_i (mod 65521).  Row r (L bytes from p = r L) adds
// S_r = sum d_j and (N - p - L) S_r + U_r with U_r = sum_j (L - j) d_j (rgb_filter_kernel).  grid nm, 64 threads
__global__ __launch_bounds__(64) void rgb_frame_kernel(const unsigned long long* __restrict__ meta, const uint32_t* __restrict__ adler,
                                                       unsigned char* __restrict__ out, int h, int w) {
    __shared__ unsigned long long sA[64], sB[64];
    const int m = blockIdx.x, lane = threadIdx.x;
    const unsigned long long* mt = meta + (size_t)m * MT_N;
    const unsigned long long off = mt[MT_OFF0];
    if (off == ~0ull) return;
    const unsigned long long L = (unsigned long long)w * 3 + 1;
    const unsigned long long Lm = L % PNG_ADLER_MOD;
    unsigned long long A = 0, Bs = 0;
    for (int y = lane; y < h; y += 64) {
        const uint32_t* d = adler + ((size_t)m * h + y) * 2;
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
    f[24] = 8; f[25] = 2; f[26] = 0; f[27] = 0; f[28] = 0;
    put_be32(f + 29, crc_bytes_slow(0u, f + 12, 17));
    const unsigned long long bytes = (mt[MT_BITS0] + 7) >> 3;
    put_be32(f + 33, (uint32_t)(2 + bytes + 4));
    f[37] = 'I'; f[38] = 'D'; f[39] = 'A'; f[40] = 'T';
    f[41] = 0x78; f[42] = 0x9c;
    unsigned char* e = f + 43 + bytes;
    put_be32(e, (b32 << 16) | a32);
    // e + 4: the IDAT CRC (png_stage_crc); then IEND
    put_be32(e + 8, 0u);
    e[12] = 'I'; e[13] = 'E'; e[14] = 'N'; e[15] = 'D';
    put_be32(e + 16, 0xae426082u);
}

}  // namespace

hipError_t launch_blend_labels(const uint8_t* images, const uint8_t* maps, const uint8_t* lut, float alpha, uint8_t* out, int n, int h,
                               int w, hipStream_t st) {
    if (n < 1 || h < 1 || w < 1 || !(alpha >= 0.f && alpha <= 1.f)) return hipErrorInvalidValue;
    const size_t total = (size_t)n * h * w;
    const bool wide = (((uintptr_t)images | (uintptr_t)maps | (uintptr_t)out) & 15) == 0;
    const size_t nvec = wide ? total / BLEND_PX : 0;
    const size_t work = nvec > total - nvec * BLEND_PX ? nvec : total - nvec * BLEND_PX;
    size_t blocks = (work + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 8192) blocks = 8192;                                // grid-stride beyond: 256 CUs x 32 blocks
    blend_labels_kernel<<<(unsigned)blocks, 256, 0, st>>>(images, maps, lut, alpha, out, nvec, total);
    return hipGetLastError();
}

size_t png_rgb_scratch_bytes(int n, int h, int w) {
    const int nm = n < PNG_MAPS ? n : PNG_MAPS;
    size_t bytes = 0;
    rgb_carve(nullptr, nm, h, w, &bytes);
    return bytes;
}

size_t png_rgb_worst_file_bytes(int h, int w) {
    // an optimal prefix code over the <= 257 symbols of a block (256 literals + end-of-block) costs no more than the 9-bit fixed code:
    // <= 9 bits per filtered byte + 9 for the end-of-block code + <= 4498 bits of header per block; 63 bytes of framing
    const size_t N = ((size_t)3 * w + 1) * h, B = (N + (1u << PNG_BLOCK_SHIFT) - 1) >> PNG_BLOCK_SHIFT;
    return 63 + (9 * N + B * (4498 + 9) + 7) / 8;
}

hipError_t launch_png_encode_rgb(const uint8_t* rgb, int n, int h, int w, int filter, void* scratch, unsigned char* out,
                                 long long out_cap, long long* cursor, long long* table, hipStream_t st) {
    if (n < 1 || h < 1 || w < 1 || h > 65536 || w > 65536 || ((size_t)3 * w + 1) * h > 0x7fffffffull || filter < -1 || filter > 4)
        return hipErrorInvalidValue;
    // the CRC grid covers every length the length-limited codes can reach: 15 bits per symbol
    const size_t N = ((size_t)3 * w + 1) * h;
    const size_t longest = 63 + (15 * (N + ((N + (1u << PNG_BLOCK_SHIFT) - 1) >> PNG_BLOCK_SHIFT)) + 7) / 8 + 4498 / 8 + 1;
    for (int p0 = 0; p0 < n; p0 += PNG_MAPS) {
        const int nm = n - p0 < PNG_MAPS ? n - p0 : PNG_MAPS;
        const RgbLayout L = rgb_carve(scratch, nm, h, w, nullptr);
        const uint8_t* src = rgb + (size_t)p0 * h * w * 3;
        const unsigned C = (unsigned)L.S.C;
        hipError_t err;
        if ((err = hipMemsetAsync(L.S.meta, 0, (size_t)nm * MT_N * 8, st)) != hipSuccess) return err;
        if ((err = hipMemsetAsync(L.S.hist, 0, (size_t)nm * L.S.B * 2 * PNG_NSYM * 4, st)) != hipSuccess) return err;
        rgb_filter_kernel<<<dim3(h, nm), 256, 0, st>>>(src, L.filt, L.adler, L.S.meta, h, w, filter, L.N, L.stride);
        rgb_hist_kernel<<<dim3(C, nm), PNG_CHUNK, 0, st>>>(L.filt, L.S.hist, L.N, L.stride, L.S.B);
        png_stage_tables(L.S, nm, 1, st);
        rgb_chunkbits_kernel<<<dim3(C, nm), PNG_CHUNK, 0, st>>>(L.filt, L.S.tables, L.S.chunkbits, L.N, L.stride, L.S.B, L.S.C);
        png_stage_offsets(L.S, nm, 1, st);
        rgb_place_kernel<<<1, 64, 0, st>>>(L.S.meta, nm, out_cap, cursor, table + (size_t)p0 * 2);
        png_stage_zero(L.S, out, nm, 1, st);
        rgb_pack_kernel<<<dim3(C, nm), PNG_CHUNK, 0, st>>>(L.filt, L.S.meta, L.S.tables, L.S.chunkoff, out, L.N, L.stride, L.S.B, L.S.C);
        png_stage_headers(L.S, out, nm, 1, st);
        rgb_frame_kernel<<<nm, 64, 0, st>>>(L.S.meta, L.adler, out, h, w);
        png_stage_crc(L.S, out, nm, 1, longest, st);
        if ((err = hipGetLastError()) != hipSuccess) return err;
    }
    return hipSuccess;
}
