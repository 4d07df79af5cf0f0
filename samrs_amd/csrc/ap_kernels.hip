// ap_kernels.hip -- the evaluation end of the instance chain: COCO mask AP needs every prediction of an image against every ground
// truth of it, not only the diagonal samrs_gt_match counts (gfx950).  Three steps, all integer until the one division per pair:
//   bit planes     a mask as uint64 [words], words = ceil(h w / 64), pixel p (row-major) = bit p % 64 of word p / 64, the unused
//                  high bits of the last word zero.  8x smaller than the mask bytes, so a tile's planes can be kept while its
//                  masks come and go a decode chunk at a time.
//     pack_bits_vec_kernel  h w % 16 == 0 and 16-byte aligned masks: a lane reads 16 pixels as one uint4 and folds them to 16
//                           bits, four neighbouring lanes make a word (two shuffles).
//     pack_bits_kernel      any size / alignment: a wave owns 64 pixels, one __ballot of mask[p] != 0 is the word.
//     label_pack_kernel     ground truth straight from the label image: a wave keeps the RGB keys of 4 x 64 pixels in registers
//                           and compares them with every colour (LDS, 256 at a time): the image is read once per call, however
//                           many instances; lanes 0..3 store the four words of an instance as one 32-byte run.
//   pair counts    inter[i][j] = sum_k popcount(A[i][k] & B[j][k]): a GEMM over bits and tiled like one.  A block owns 64 x 64
//                  pairs and a K-range of words; 16 words of 64 + 64 planes are staged in LDS k-major ([k][plane], so the 16
//                  planes a half-wave reads at one k are consecutive 8-byte words: no bank conflict, the A side broadcasts), a
//                  thread accumulates 4 x 4 pairs in registers (8 LDS reads per 16 and + popcount) and adds its partial sums into
//                  the zeroed output with integer atomics: exact, and the same whatever the order.  Rows past na / nb and words
//                  past the K-range are staged as 0; nothing out of range is read or written.
//     bit_area_kernel       area[i] = sum_k popcount(P[i][k]), a block per plane and K-range.
//   COCO matching  COCOeval.evaluateImg's greedy matching for one image (samrs_hip.h samrs_coco_match states it): one block per
//                  area range, one wave per IoU threshold.  The block ranks the detections by counting (score descending, index
//                  ascending: a stable sort) into LDS; then every wave walks the kept detections on its own: its lanes stride over
//                  the ground truths (lane g % 64 owns ground truth g, also its matched flag, so no flag is shared between
//                  lanes), keep the best not-yet-matched candidate of the non-ignored and of the ignored group, and a shuffle
//                  butterfly picks the winner: greatest IoU, the later ground truth on a tie.
//                  IoU = inter / union as a correctly rounded double (iou_rn: the compiled quotient, then one exact-residual
//                  step that moves it to the neighbouring double where that one is nearer), so `iou >= threshold` and the
//                  comparison of two IoUs decide exactly as IEEE division does on the host.
#include "common.h"
#include "kernels.h"

namespace {

typedef unsigned long long u64;

// byte c of w is non-zero -> bit c
__device__ __forceinline__ uint32_t pb_nz4(uint32_t w) {
    const uint32_t f = ((((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u) >> 7;      // bits 0, 8, 16, 24
    return (f | (f >> 7) | (f >> 14) | (f >> 21)) & 0xFu;
}

// thread t of grid.x: the 16 pixels 16 t .. 16 t + 15 (all inside or all outside: hw % 16 == 0); grid.y strides over the masks
__global__ __launch_bounds__(256) void pack_bits_vec_kernel(const uint8_t* __restrict__ masks, int n, long hw, long words,
                                                            u64* __restrict__ out) {
    const long grp = (long)blockIdx.x * 256 + threadIdx.x;
    const long p0 = grp * 16, wd = grp >> 2;
    const int sh = 16 * (threadIdx.x & 3);
    for (int j = blockIdx.y; j < n; j += gridDim.y) {
        uint32_t bits = 0u;
        if (p0 < hw) {
            const uint4 m = *reinterpret_cast<const uint4*>(masks + (size_t)j * hw + p0);
            bits = pb_nz4(m.x) | (pb_nz4(m.y) << 4) | (pb_nz4(m.z) << 8) | (pb_nz4(m.w) << 12);
        }
        u64 v = (u64)bits << sh;
        v |= __shfl_xor(v, 1, 64);
        v |= __shfl_xor(v, 2, 64);
        if ((threadIdx.x & 3) == 0 && wd < words) out[(size_t)j * words + wd] = v;
    }
}

// wave v of grid.x: the 64 pixels of word v
__global__ __launch_bounds__(256) void pack_bits_kernel(const uint8_t* __restrict__ masks, int n, long hw, long words,
                                                        u64* __restrict__ out) {
    const long wd = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const long p = wd * 64 + lane;
    for (int j = blockIdx.y; j < n; j += gridDim.y) {
        const bool set = p < hw && masks[(size_t)j * hw + p] != 0;
        const u64 b = __ballot(set);
        if (lane == 0 && wd < words) out[(size_t)j * words + wd] = b;
    }
}

constexpr int LP_WPW = 4;           // words per wave
constexpr int LP_COLORS = 256;      // colours per LDS round
static_assert(LP_WPW == 4, "lanes 0..3 store the four words of an instance");

// wave v of the grid: the words 4 v .. 4 v + 3.  A pixel outside the image has the key 0xFFFFFFFF, which no colour has.
__global__ __launch_bounds__(256) void label_pack_kernel(const uint8_t* __restrict__ label, const uint8_t* __restrict__ colors, int n,
                                                         long hw, long words, u64* __restrict__ out) {
    __shared__ uint32_t col_s[LP_COLORS];
    const long w0 = (((long)blockIdx.x * 256 + threadIdx.x) >> 6) * LP_WPW;
    const int lane = threadIdx.x & 63;
    uint32_t key[LP_WPW];
#pragma unroll
    for (int q = 0; q < LP_WPW; ++q) {
        const long p = (w0 + q) * 64 + lane;
        key[q] = 0xFFFFFFFFu;
        if (p < hw) {
            const uint8_t* px = label + 3 * (size_t)p;
            key[q] = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
        }
    }
    for (int j0 = 0; j0 < n; j0 += LP_COLORS) {
        const int m = n - j0 < LP_COLORS ? n - j0 : LP_COLORS;
        __syncthreads();
        if ((int)threadIdx.x < m) {
            const uint8_t* c = colors + 3 * (size_t)(j0 + threadIdx.x);
            col_s[threadIdx.x] = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
        }
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const uint32_t c = col_s[k];
            const u64 b0 = __ballot(key[0] == c), b1 = __ballot(key[1] == c), b2 = __ballot(key[2] == c), b3 = __ballot(key[3] == c);
            const u64 v = lane == 0 ? b0 : lane == 1 ? b1 : lane == 2 ? b2 : b3;
            if (lane < LP_WPW && w0 + lane < words) out[(size_t)(j0 + k) * words + w0 + lane] = v;
        }
    }
}

constexpr int PC_T = 64;        // pairs tile: PC_T x PC_T
constexpr int PC_KS = 16;       // words staged per step
constexpr int PC_R = PC_T / 16; // pairs per thread and side
static_assert(PC_T * PC_KS == 4 * 256, "a thread stages four words of each side per step");

// grid (ceil(nb / 64), ceil(na / 64), K-ranges of kchunk words); kchunk % PC_KS == 0 and kchunk * 64 < 2^32
__global__ __launch_bounds__(256) void pair_counts_kernel(const u64* __restrict__ A, int na, const u64* __restrict__ B, int nb, long words,
                                                          long kchunk, u64* __restrict__ inter) {
    __shared__ u64 a_s[PC_KS][PC_T + 1], b_s[PC_KS][PC_T + 1];
    const int i0 = blockIdx.y * PC_T, j0 = blockIdx.x * PC_T;
    const long k_lo = (long)blockIdx.z * kchunk;
    const long k_hi = k_lo + kchunk < words ? k_lo + kchunk : words;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;      // pairs (ty + 16 x, tx + 16 y); staging: word tx of rows ty + 16 m
    uint32_t acc[PC_R][PC_R];
#pragma unroll
    for (int x = 0; x < PC_R; ++x)
#pragma unroll
        for (int y = 0; y < PC_R; ++y) acc[x][y] = 0u;
    for (long k0 = k_lo; k0 < k_hi; k0 += PC_KS) {
        u64 av[PC_R], bv[PC_R];
        const long k = k0 + tx;
#pragma unroll
        for (int m = 0; m < PC_R; ++m) {
            const int r = ty + 16 * m;
            av[m] = (i0 + r < na && k < k_hi) ? A[(size_t)(i0 + r) * words + k] : 0ull;
            bv[m] = (j0 + r < nb && k < k_hi) ? B[(size_t)(j0 + r) * words + k] : 0ull;
        }
        __syncthreads();                                         // the last step's reads are done
#pragma unroll
        for (int m = 0; m < PC_R; ++m) {
            a_s[tx][ty + 16 * m] = av[m];
            b_s[tx][ty + 16 * m] = bv[m];
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < PC_KS; ++kk) {
            u64 a[PC_R], b[PC_R];
#pragma unroll
            for (int x = 0; x < PC_R; ++x) a[x] = a_s[kk][ty + 16 * x];
#pragma unroll
            for (int y = 0; y < PC_R; ++y) b[y] = b_s[kk][tx + 16 * y];
#pragma unroll
            for (int x = 0; x < PC_R; ++x)
#pragma unroll
                for (int y = 0; y < PC_R; ++y) acc[x][y] += (uint32_t)__popcll(a[x] & b[y]);
        }
    }
#pragma unroll
    for (int x = 0; x < PC_R; ++x)
#pragma unroll
        for (int y = 0; y < PC_R; ++y) {
            const int i = i0 + ty + 16 * x, j = j0 + tx + 16 * y;
            if (i < na && j < nb && acc[x][y]) atomicAdd(&inter[(size_t)i * nb + j], (u64)acc[x][y]);
        }
}

// grid (n, K-ranges of kchunk words): one atomic per block into the zeroed area
__global__ __launch_bounds__(256) void bit_area_kernel(const u64* __restrict__ P, long words, long kchunk, u64* __restrict__ area) {
    __shared__ unsigned int part_s[4];
    const long k_lo = (long)blockIdx.y * kchunk;
    const long k_hi = k_lo + kchunk < words ? k_lo + kchunk : words;
    const u64* row = P + (size_t)blockIdx.x * words;
    unsigned int cnt = 0u;
    for (long k = k_lo + threadIdx.x; k < k_hi; k += 256) cnt += (unsigned int)__popcll(row[k]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((threadIdx.x & 63) == 0) part_s[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 c = (u64)part_s[0] + part_s[1] + part_s[2] + part_s[3];
        if (c) atomicAdd(&area[blockIdx.x], c);
    }
}

// inter / uni (0 < inter <= uni < 2^31, both exact as doubles) rounded to nearest.  q is the compiled quotient; r = inter - q uni is
// exact in one fma when q is within an ulp of the true quotient, and the neighbour of q on r's side is taken where its own exact
// residual is smaller.  A quotient of two such integers never lies halfway between two doubles, so no tie rule is needed.
__device__ __forceinline__ double iou_rn(long long inter, long long uni) {
    const double a = (double)inter, b = (double)uni;
    double q = a / b;
    const double r = fma(-q, b, a);
    if (r != 0.0) {
        const double q2 = __longlong_as_double(__double_as_longlong(q) + (r > 0.0 ? 1 : -1));
        const double r2 = fma(-q2, b, a);
        if (fabs(r2) < fabs(r)) q = q2;
    }
    return q;
}

struct Cand { double iou; int g; };
__device__ __forceinline__ void cand_reduce(Cand& c) {         // greatest IoU, then the later ground truth; g < 0 = none
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double oi = __shfl_xor(c.iou, off, 64);
        const int og = __shfl_xor(c.g, off, 64);
        if (og >= 0 && (c.g < 0 || oi > c.iou || (oi == c.iou && og > c.g))) {
            c.iou = oi;
            c.g = og;
        }
    }
}

// grid = area ranges, block = 64 T threads, dynamic LDS = max_det ints.  gmatched: zeroed bytes [A][T][ng].
// MIN (samrs_coco_match_min): a second triple of counts, those of the masks' boundary bands, and the pair's score is the smaller of
// the two IoUs; areas, ignore flags and everything else stay the first triple's.  Without MIN the second triple is not looked at.
template <bool MIN>
__global__ void coco_match_kernel(const long long* __restrict__ inter, const long long* __restrict__ area_d,
                                  const long long* __restrict__ area_g, const long long* __restrict__ inter_b,
                                  const long long* __restrict__ area_db, const long long* __restrict__ area_gb,
                                  const float* __restrict__ scores, int nd, int ng, CocoMatchParams P,
                                  int T, int max_det, uint8_t* __restrict__ gmatched, int32_t* __restrict__ order_out,
                                  int32_t* __restrict__ match_out, uint8_t* __restrict__ ign_out, int32_t* __restrict__ n_valid_out,
                                  int32_t* __restrict__ n_kept_out) {
    extern __shared__ int order_s[];
    __shared__ int nvalid_s;
    const int a = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const double lo = P.lo[a], hi = P.hi[a];
    int bad = 0;
    for (int d = tid; d < nd; d += nthr) bad |= scores[d] != scores[d] ? 1 : 0;
    bad = __syncthreads_or(bad);
    const int n_kept = bad ? -1 : (nd < max_det ? nd : max_det);
    for (int r = tid; r < T * max_det; r += nthr) {
        match_out[(size_t)a * T * max_det + r] = -1;
        ign_out[(size_t)a * T * max_det + r] = 0;
    }
    for (int r = tid; r < max_det; r += nthr) {
        order_s[r] = -1;
        if (a == 0) order_out[r] = -1;
    }
    if (tid == 0) {
        nvalid_s = 0;
        if (a == 0) *n_kept_out = n_kept;
    }
    __syncthreads();
    int cnt = 0;
    for (int g = tid; g < ng; g += nthr) {
        const double ag = (double)area_g[g];
        cnt += !(ag < lo || ag > hi) ? 1 : 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if ((tid & 63) == 0 && cnt) atomicAdd(&nvalid_s, cnt);
    if (!bad) {
        // rank by counting: d precedes e iff score[d] > score[e], or the scores are equal and d < e
        for (int d = tid; d < nd; d += nthr) {
            const float s = scores[d];
            int rank = 0;
            for (int e = 0; e < nd; ++e) {
                const float se = scores[e];
                rank += (se > s || (se == s && e < d)) ? 1 : 0;
            }
            if (rank < max_det) {
                order_s[rank] = d;
                if (a == 0) order_out[rank] = d;
            }
        }
    }
    __syncthreads();
    if (tid == 0) n_valid_out[a] = nvalid_s;
    if (bad) return;

    const int t = tid >> 6, lane = tid & 63;
    const double bar = P.bar[t];
    uint8_t* gm = gmatched + ((size_t)a * T + t) * ng;
    for (int r = 0; r < n_kept; ++r) {
        const int d = order_s[r];
        const long long ad = area_d[d];
        const long long* row = inter + (size_t)d * ng;
        Cand cv{bar, -1}, ci{bar, -1};                           // non-ignored / ignored ground truths
        for (int g = lane; g < ng; g += 64) {
            if (gm[g]) continue;
            const long long ag = area_g[g], in = row[g], un = ad + ag - in;
            double iou = (un > 0 && in > 0) ? iou_rn(in, un) : 0.0;
            if constexpr (MIN) {
                const long long inb = inter_b[(size_t)d * ng + g], unb = area_db[d] + area_gb[g] - inb;
                const double iou_b = (unb > 0 && inb > 0) ? iou_rn(inb, unb) : 0.0;
                iou = iou_b < iou ? iou_b : iou;
            }
            const bool ig = (double)ag < lo || (double)ag > hi;
            Cand& c = ig ? ci : cv;
            if (iou >= c.iou) {                                  // ascending g: the later one on a tie
                c.iou = iou;
                c.g = g;
            }
        }
        cand_reduce(cv);
        cand_reduce(ci);
        const int m = cv.g >= 0 ? cv.g : ci.g;
        const bool m_ign = cv.g < 0 && ci.g >= 0;
        if (m >= 0 && lane == (m & 63)) gm[m] = 1;               // the lane that owns ground truth m
        if (lane == 0) {
            const size_t o = ((size_t)a * T + t) * max_det + r;
            match_out[o] = m;
            ign_out[o] = m >= 0 ? (m_ign ? 1 : 0) : (((double)ad < lo || (double)ad > hi) ? 1 : 0);
        }
    }
}

long pick_kchunk(long words, long blocks_per_range, long want_blocks, long step) {
    long parts = want_blocks / (blocks_per_range > 0 ? blocks_per_range : 1);
    parts = parts < 1 ? 1 : (parts > 1024 ? 1024 : parts);
    long kchunk = (words + parts - 1) / parts;
    kchunk = (kchunk + step - 1) / step * step;
    return kchunk < step ? step : kchunk;
}

}  // namespace

hipError_t launch_pack_bits(const uint8_t* masks, int n, int h, int w, unsigned long long* out, hipStream_t s) {
    if (!masks || !out || n < 1 || h < 1 || w < 1 || (long)h * w >= (1l << 30)) return hipErrorInvalidValue;
    const long hw = (long)h * w, words = (hw + 63) / 64;
    const unsigned gy = n < 65535 ? n : 65535;
    if (hw % 16 == 0 && (((uintptr_t)masks) & 15) == 0) {
        const unsigned gx = (unsigned)((hw / 16 + 255) / 256);
        pack_bits_vec_kernel<<<dim3(gx, gy), 256, 0, s>>>(masks, n, hw, words, out);
    } else {
        const unsigned gx = (unsigned)((words + 3) / 4);
        pack_bits_kernel<<<dim3(gx, gy), 256, 0, s>>>(masks, n, hw, words, out);
    }
    return hipGetLastError();
}

hipError_t launch_label_pack_bits(const uint8_t* label_rgb, const uint8_t* colors, int n, int h, int w, unsigned long long* out,
                                  hipStream_t s) {
    if (!label_rgb || !colors || !out || n < 1 || h < 1 || w < 1 || (long)h * w >= (1l << 30)) return hipErrorInvalidValue;
    const long hw = (long)h * w, words = (hw + 63) / 64;
    const unsigned gx = (unsigned)((words + 4 * LP_WPW - 1) / (4 * LP_WPW));
    label_pack_kernel<<<gx, 256, 0, s>>>(label_rgb, colors, n, hw, words, out);
    return hipGetLastError();
}

hipError_t launch_bit_areas(const unsigned long long* planes, int n, long words, unsigned long long* area, hipStream_t s) {
    if (!planes || !area || n < 1 || words < 1 || words > (1l << 24)) return hipErrorInvalidValue;
    HIP_CHECK_RET(hipMemsetAsync(area, 0, sizeof(unsigned long long) * (size_t)n, s));
    const long kchunk = pick_kchunk(words, n, 1024, 256);
    bit_area_kernel<<<dim3((unsigned)n, (unsigned)((words + kchunk - 1) / kchunk)), 256, 0, s>>>(planes, words, kchunk, area);
    return hipGetLastError();
}

hipError_t launch_pair_counts(const unsigned long long* a, int na, const unsigned long long* b, int nb, long words,
                              unsigned long long* inter, hipStream_t s) {
    if (!a || !b || !inter || na < 1 || nb < 1 || words < 1 || words > (1l << 24)) return hipErrorInvalidValue;
    HIP_CHECK_RET(hipMemsetAsync(inter, 0, sizeof(unsigned long long) * (size_t)na * nb, s));
    const long gx = (nb + PC_T - 1) / PC_T, gy = (na + PC_T - 1) / PC_T;
    if (gx > 65535 || gy > 65535) return hipErrorInvalidValue;
    const long kchunk = pick_kchunk(words, gx * gy, 1024, PC_KS);                 // <= 2^24 words: kchunk * 64 < 2^32
    pair_counts_kernel<<<dim3((unsigned)gx, (unsigned)gy, (unsigned)((words + kchunk - 1) / kchunk)), 256, 0, s>>>(a, na, b, nb, words,
                                                                                                                 kchunk, inter);
    return hipGetLastError();
}

size_t coco_match_scratch_bytes(int ng, int n_thresholds, int n_ranges) {
    return (((size_t)(ng > 0 ? ng : 1) * n_thresholds * n_ranges) + 15) / 16 * 16;
}

hipError_t launch_coco_match(const long long* inter, const long long* area_d, const long long* area_g, const long long* inter_b,
                             const long long* area_db, const long long* area_gb, const float* scores, int nd, int ng, const CocoMatchParams& P, int n_thresholds, int n_ranges, int max_det, void* scratch, int32_t* order_out,
                             int32_t* match_out, uint8_t* ign_out, int32_t* n_valid_out, int32_t* n_kept_out, hipStream_t s) {
    if (nd < 0 || ng < 0 || n_thresholds < 1 || n_thresholds > COCO_MAX_THRESHOLDS || n_ranges < 1 || n_ranges > COCO_MAX_RANGES ||
        max_det < 1 || max_det > COCO_MAX_DET || !scratch || !order_out || !match_out || !ign_out || !n_valid_out || !n_kept_out)
        return hipErrorInvalidValue;
    if ((nd > 0 && (!scores || !area_d)) || (ng > 0 && !area_g) || (nd > 0 && ng > 0 && !inter)) return hipErrorInvalidValue;
    const bool with_min = inter_b || area_db || area_gb;       // the band triple: all of it where the first triple is needed, or none
    if (with_min && ((nd > 0 && !area_db) || (ng > 0 && !area_gb) || (nd > 0 && ng > 0 && !inter_b))) return hipErrorInvalidValue;
    HIP_CHECK_RET(hipMemsetAsync(scratch, 0, coco_match_scratch_bytes(ng, n_thresholds, n_ranges), s));
    const size_t lds = sizeof(int) * (size_t)max_det;
    if (with_min)
        coco_match_kernel<true><<<n_ranges, 64 * n_thresholds, lds, s>>>(inter, area_d, area_g, inter_b, area_db, area_gb, scores, nd, ng, P,
                                                                         n_thresholds, max_det, (uint8_t*)scratch, order_out, match_out,
                                                                         ign_out, n_valid_out, n_kept_out);
    else
        coco_match_kernel<false><<<n_ranges, 64 * n_thresholds, lds, s>>>(inter, area_d, area_g, nullptr, nullptr, nullptr, scores, nd, ng, P,
                                                                          n_thresholds, max_det, (uint8_t*)scratch, order_out, match_out,
                                                                          ign_out, n_valid_out, n_kept_out);
    return hipGetLastError();
}
