// png_device.h -- what the two on-device PNG encoders share: png_kernels.hip (the gray + palette files of a class map) and
// overlay_kernels.hip (a truecolour file of arbitrary pixels).  Constants of the common scratch layout, the per-file meta block, and
// the device functions both use: block scan, file length, big-endian stores and the CRC by GF(2) shifts.  The stages that do not look
// at tokens (code tables and block headers, chunk offsets, zeroing, headers, CRC) are png_kernels.hip's kernels themselves, launched
// for one stream per file through the png_stage_* functions of kernels.h.  Everything here is in an unnamed namespace: each of the
// two sources gets its own copy, inlined into its own kernels.
#pragma once
#include "common.h"

namespace {

constexpr int PNG_MAPS = 8;                      // maps per pass: bounds the scratch (8 bytes per token slot per map)
constexpr int PNG_CHUNK = 1024;                  // tokens per chunk (= threads of the chunk kernels)
constexpr int PNG_BLOCK_SHIFT = 20;              // parse tokens per deflate block: 2^20, as the host encoder
constexpr int PNG_CHUNKS_PER_BLOCK = 1 << (PNG_BLOCK_SHIFT - 10);
constexpr int PNG_NSYM = 316;                    // 286 literal / length + 30 distance symbols
constexpr int PNG_HDR_WORDS = 160;               // <= 3 + 14 + 19 * 3 + 316 * 14 = 4498 bits of block header
constexpr int PNG_CRC_PIECE = 256;               // IDAT bytes per thread of the CRC kernel
constexpr uint32_t PNG_ADLER_MOD = 65521u;

// per-map values in the meta block (uint64 each)
enum { MT_NTOK, MT_NBLK, MT_NCHUNK, MT_BITS0, MT_BITS1, MT_OFF0, MT_OFF1, MT_LEN0, MT_LEN1, MT_CRC0, MT_CRC1, MT_N = 16 };

__host__ __device__ inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* sm /*[17]*/, uint32_t* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    __syncthreads();
    if (lane == 63) sm[wave] = inc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int i = 0; i < nw; ++i) { const uint32_t t = sm[i]; sm[i] = run; run += t; }
        sm[16] = run;
    }
    __syncthreads();
    *total = sm[16];
    return sm[wave] + inc - v;
}

// ---- placement ---------------------------------------------------------------------------------------------------------------
// file = signature 8 + IHDR 25 + IDAT (12 + 2 + deflate bytes + 4) + IEND 12
__device__ __forceinline__ long long png_file_len(unsigned long long bits) { return 63 + (long long)((bits + 7) >> 3); }

// ---- CRC-32 helpers (reflected polynomial 0xedb88320; multmodp / x2nmodp as zlib's crc32.c) ------------------------------------
__device__ __forceinline__ uint32_t crc_mult(uint32_t a, uint32_t b) {     // a * b mod P; a != 0
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = b & 1 ? (b >> 1) ^ 0xedb88320u : b >> 1;
    }
    return p;
}
__device__ uint32_t crc_x8n(unsigned long long n) {               // x^(8 n) mod P
    uint32_t p = 1u << 31, x2k = 1u << 30;                        // x^0; x^(2^k) for k = 0
    for (int k = 0; k < 3; ++k) x2k = crc_mult(x2k, x2k);         // x^8
    while (n) {
        if (n & 1) p = crc_mult(x2k, p);
        n >>= 1;
        x2k = crc_mult(x2k, x2k);
    }
    return p;
}
__device__ uint32_t crc_bytes_slow(uint32_t c, const unsigned char* p, int n) {   // standard CRC-32 update, bitwise
    c = ~c;
    for (int i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = c & 1 ? (c >> 1) ^ 0xedb88320u : c >> 1;
    }
    return ~c;
}

__device__ __forceinline__ void put_be32(unsigned char* p, uint32_t v) {
    p[0] = (unsigned char)(v >> 24); p[1] = (unsigned char)(v >> 16); p[2] = (unsigned char)(v >> 8); p[3] = (unsigned char)v;
}

}  // namespace
