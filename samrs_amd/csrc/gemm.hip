// gemm.hip -- MFMA GEMMs for the SAM hot path (gfx950).
//
//   gemm_et  : C[M,N] = A[M,K] * B[N,K]^T (+bias[n]) (+add2d[m % period, n]) (+C) (GELU)
//              A, B in the MFMA operand type (bf16 / f16), fp32 accumulate.
//              Replaces every nn.Linear / 1x1 conv / ConvTranspose-as-GEMM on the image side:
//              qkv / proj (modeling/image_encoder.py:227,238), MLP lin1/lin2 (common.py:25-26),
//              patch embed (image_encoder.py:387-395), neck (image_encoder.py:88-104), decoder
//              image-side projections (transformer.py:203-206) and the upscaler
//              (mask_decoder.py:53-59).
//   gemm_f32 : exact-fp32 GEMM on v_mfma_f32_16x16x4_f32 for the token side of the decoder
//              (a few hundred rows; precision matters more than rate there).
//
// gemm_et structure (v1): 128x128x64 block tile, 256 threads = 4 waves (2x2), each wave a 64x64
// sub-tile as 4x4 MFMA 16x16x32 tiles; operands staged global -> VGPR -> LDS with a one-tile
// register prefetch (issue loads for tile t+1 before computing tile t, write them after); LDS
// rows are 128 B with an XOR swizzle of the 16-byte chunk index so that ds_read_b128 fragment
// reads are bank-conflict free.  MFMA operands are swapped (first = weight fragment, second =
// activation fragment) so that each lane ends up with 4 CONSECUTIVE output columns of one row:
// the epilogue then uses 8-byte (ET) / 16-byte (fp32) vector accesses and float4 bias loads.
//
// One translation unit per kernel family.  This one keeps the dispatch (launch_gemm_et: validate -> gemm_select -> one switch), the
// process state the selection rule reads, the dominant kernel (four-wave 256x256 gemm_et_w4x_kernel) and the eight-wave kernels on
// 256-row tiles -- gemm_et_big_kernel, gemm_et_x64_kernel, gemm_et_x64p_kernel, gemm_et_mx_kernel -- which share instantiations of
// epilogue_pair_et and must be compiled together (the optimizer shapes a caller by the other callers of an internal function it sees:
// apart, two of them get other registers and spills; tools/device_code_diff.py, profiles/r12_gemm_split.txt).  Elsewhere:
//   gemm_ring.hip        gemm_et_kernel (the v1 kernel above, 128 x 128) and gemm_et_stag_kernel (256 x 128, 3-stage ring)
//   gemm_dual.hip        gemm_et_dual_kernel: 2 blocks / CU; the GELU(LayerNorm2d) launcher
//   gemm_decoder.hip     gemm_et_k256_kernel (K = 256 streaming) and gemm_f32_kernel (exact fp32)
//   gemm_experiments.hip make EXPERIMENTS=1 only: gemm_et_m32_kernel, gemm_et_w4_kernel, the LayerNorm fold's two public launchers
//   gemm_device.h        device helpers that more than one file uses;  gemm_families.h: the launchers of the other files
#include "gemm_device.h"
#include "gemm_families.h"


// CUs of the current device: the grid of a persistent kernel.  cu_count() asks once per process (the first launch's device; the
// devices of one box are the same part); the launchers that always asked per call go on doing so (cu_count_now()), since engines of
// one process may sit on different devices (DeviceGuard).
int gemm_fam::cu_count_now() {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
}
int gemm_fam::cu_count() {
    static const int n = cu_count_now();
    return n;
}

namespace {


// ---------------------------------------------------------------------------------------------
// ET-output epilogue of the 256x320 kernel (NI = 5).  A wave's sub-tile is 80 columns = 160 bytes per row:
// stored per wave, the row segments straddle 64-byte sectors and the generic code spills.  Here the two waves
// that sit side by side (wn = 2p, 2p+1: 160 columns = 320 bytes, 64-byte aligned) bounce through ONE shared
// LDS buffer and each stores half of the rows as full 320-byte segments (20 lanes x 16 B per row).
// Block-wide barriers: all 8 waves are past the main loop here (the stagger has been re-aligned).
//   acc[i][j]: n-tile i (16 cols), m-tile j (16 rows); 8 m-tiles, 4 per pass.
// ---------------------------------------------------------------------------------------------
// FOLD (LayerNorm folded into this GEMM, see gemm_et_x64p_kernel): the value is rstd_m * acc + (-rstd_m mean_m) * cvec_n +
// bias_n with (rstd_m, -rstd_m mean_m) = rowstat[m] (global, written by ln_rowstat_kernel) instead of acc + bias_n.
// MXO (round 4): the output is also the A operand of a GEMM whose lo terms run on MXFP4 (lin1 -> lin2 in the all-split mode): besides
// the ET row segments the epilogue writes hi / lo of every value as fp4 codes + E8M0 scales on a K axis padded per WAVE TILE (80 -> 96
// columns: a 32-element block never straddles two waves; mx4_pack_kernel perm 2 lays the weights out the same way).  The 16 columns of
// n-tile i of a row sit in the 4 lanes fq = 0..3 (4 each): block 0 = n-tiles 0 | 1, block 1 = 2 | 3, block 2 = 4 | zeros; block maxima
// by two cross-lane swaps (l ^ 16, l ^ 32), codes by v_cvt_scalef32_pk_fp4_f32, one dword store per lane, block and tensor (position
// 8 fq + 4 (i & 1) + e of the block holds column 16 (i & 1) + 4 fq + e).
// GELU: 0 none, 1 the fp32-epsilon erf (common.h gelu_erf2), 2 the cheaper erf of the 1x-rate mode (gelu_erf2_et)
template <int PREC, int GELU, int JC = 4, bool DRAIN = false, bool FOLD = false, bool MXO = false, bool STREAM = false /* non-temporal ET stores */>
__device__ __forceinline__ void epilogue_pair_et(f32x4_t (&acc)[5][8], unsigned char* lds, void* __restrict__ Cv,
                                                 const float* __restrict__ bias, const float* __restrict__ pre2d, int period, int N,
                                                 int m_base /* wave tile row 0 */, int n_pair /* first column of the pair */,
                                                 int wm, int wn, int lane, const float2* __restrict__ rowstat = nullptr /* FOLD: [M] */,
                                                 const float* __restrict__ cvec = nullptr /* FOLD */, MxOut mxo = MxOut()) {
    constexpr int RS = 400;                 // 320 data bytes + pad: 100 words = 4 (mod 32)
    constexpr int TS = 16 * RS;
    const int fr = lane & 15, fq = lane >> 4, half = wn & 1;
    unsigned char* scr = lds + (wm * 2 + (wn >> 1)) * (JC * TS);
    float4 bv[5];
#pragma unroll
    for (int i = 0; i < 5; ++i)
        bv[i] = bias ? *reinterpret_cast<const float4*>(bias + n_pair + half * 80 + i * 16 + 4 * fq) : make_float4(0.f, 0.f, 0.f, 0.f);
    // FOLD: (rstd, -rstd mean) of this lane's rows, one pass ahead (global, 8 bytes per row: L2 hits next to the bias loads)
    float2 rs_cur[JC], rs_nxt[JC];
    if constexpr (FOLD) {
#pragma unroll
        for (int jj = 0; jj < JC; ++jj) rs_cur[jj] = rowstat[m_base + jj * 16 + fr];
    }
#pragma unroll
    for (int j0 = 0; j0 < 8; j0 += JC) {
        if (j0) __syncthreads();
        if constexpr (FOLD) {
            if (j0 + JC < 8) {
#pragma unroll
                for (int jj = 0; jj < JC; ++jj) rs_nxt[jj] = rowstat[m_base + (j0 + JC + jj) * 16 + fr];
            }
        }
#pragma unroll
        for (int jj = 0; jj < JC; ++jj) {
            const int j = j0 + jj;
            float2 rs = make_float2(1.f, 0.f);
            if constexpr (FOLD) rs = rs_cur[jj];
            float mxh[MXO ? 24 : 1], mxl[MXO ? 24 : 1];          // MXO: hi / lo of this row's 20 values (+ 4 zeros of the padded n-tile)
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                float v0 = acc[i][j][0] + bv[i].x, v1 = acc[i][j][1] + bv[i].y;
                float v2 = acc[i][j][2] + bv[i].z, v3 = acc[i][j][3] + bv[i].w;
                if constexpr (FOLD) {
                    const float4 cv = *reinterpret_cast<const float4*>(cvec + n_pair + half * 80 + i * 16 + 4 * fq);
                    v0 = fmaf(rs.x, acc[i][j][0], fmaf(rs.y, cv.x, bv[i].x)); v1 = fmaf(rs.x, acc[i][j][1], fmaf(rs.y, cv.y, bv[i].y));
                    v2 = fmaf(rs.x, acc[i][j][2], fmaf(rs.y, cv.z, bv[i].z)); v3 = fmaf(rs.x, acc[i][j][3], fmaf(rs.y, cv.w, bv[i].w));
                }
                if (pre2d) {
                    const float4 e = *reinterpret_cast<const float4*>(pre2d + (size_t)((m_base + j * 16 + fr) % period) * N + n_pair +
                                                                      half * 80 + i * 16 + 4 * fq);
                    v0 += e.x; v1 += e.y; v2 += e.z; v3 += e.w;
                }
                if constexpr (GELU == 2) { const float2_t g01 = gelu_erf2_et(float2_t{v0, v1}), g23 = gelu_erf2_et(float2_t{v2, v3}); v0 = g01.x; v1 = g01.y; v2 = g23.x; v3 = g23.y; }
                else if constexpr (GELU != 0) { const float2_t g01 = gelu_erf2(float2_t{v0, v1}), g23 = gelu_erf2(float2_t{v2, v3}); v0 = g01.x; v1 = g01.y; v2 = g23.x; v3 = g23.y; }
                uint2 o;
                o.x = pack2<PREC>(v0, v1);
                o.y = pack2<PREC>(v2, v3);
                *reinterpret_cast<uint2*>(scr + jj * TS + fr * RS + half * 160 + (i * 16 + 4 * fq) * 2) = o;
                if constexpr (MXO) {
                    const float vv[4] = {v0, v1, v2, v3};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float hv = ET<PREC>::to_float((uint16_t)(((e & 2) ? o.y : o.x) >> (16 * (e & 1))));
                        mxh[4 * i + e] = hv;
                        mxl[4 * i + e] = vv[e] - hv;
                    }
                }
            }
            if constexpr (MXO) {
#pragma unroll
                for (int e = 20; e < 24; ++e) { mxh[e] = 0.f; mxl[e] = 0.f; }
                const int row = m_base + j * 16 + fr;
                const int wt = (n_pair + half * 80) / 80, nblk = (N / 80) * 3;
                const size_t rowb = (size_t)row * (size_t)(nblk * 16);
#pragma unroll
                for (int b3 = 0; b3 < 3; ++b3) {
                    float ah = 0.f, al = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) { ah = fmaxf(ah, fabsf(mxh[8 * b3 + e])); al = fmaxf(al, fabsf(mxl[8 * b3 + e])); }
                    ah = fmaxf(ah, lane_xor16(ah)); al = fmaxf(al, lane_xor16(al));
                    ah = fmaxf(ah, lane_xor32(ah)); al = fmaxf(al, lane_xor32(al));
                    const int bh = mx_scale_byte(ah), bl = mx_scale_byte(al);
                    const size_t at = rowb + (size_t)(wt * 3 + b3) * 16 + 4 * fq;
                    *reinterpret_cast<uint32_t*>(mxo.q_hi + at) = fp4_pack8(mxh + 8 * b3, bh);
                    *reinterpret_cast<uint32_t*>(mxo.q_lo + at) = fp4_pack8(mxl + 8 * b3, bl);
                    if (fq == 0) {
                        const size_t si = mx_scale_index(false, row, wt * 3 + b3, nblk * 32 / MXK);
                        mxo.s_hi[si] = (unsigned char)bh;
                        mxo.s_lo[si] = (unsigned char)bl;
                    }
                }
            }
        }
        if (DRAIN && j0 == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // this wave: rows 8*half .. +7 of each of the JC m-tiles = JC x 8 rows x 20 chunks = 2.5 JC passes of 64 lanes
#pragma unroll
        for (int h = 0; h < JC * 160 / 64; ++h) {
            const int idx = lane + 64 * h;
            const int jj = idx / 160, rem = idx % 160;
            const int row = 8 * half + rem / 20, ch = rem % 20;
            const uint4 v = *reinterpret_cast<const uint4*>(scr + jj * TS + row * RS + ch * 16);
            uint16_t* C = reinterpret_cast<uint16_t*>(Cv) + (size_t)(m_base + (j0 + jj) * 16 + row) * N + n_pair + ch * 8;
            store16_stream<STREAM>(C, v);
        }
        if constexpr (FOLD) {
#pragma unroll
            for (int jj = 0; jj < JC; ++jj) rs_cur[jj] = rs_nxt[jj];
        }
    }
}


// ---------------------------------------------------------------------------------------------
// gemm_et_big_kernel: 256x256x32 block tile, 8 waves as 2 (M) x 4 (N), wave tile 128x64
// (8 x 4 MFMA 16x16x32 tiles, one full K=32 step per MFMA), FOUR-stage LDS ring (4 x 32 KiB) filled
// by LDS-DMA three tiles ahead, wave groups staggered by one barrier interval (L | C segments).
// Versus the 256x128x64 kernel: 4 instead of 6 DMA pieces and 12 instead of 16 ds_read_b128 per 32
// MFMAs, and 2 instead of 4 barriers -- the per-CU vector-memory / LDS traffic per FLOP is what
// capped that kernel.
//
// LDS rows are 64 B (32 ET): four rows per 256-B bank row, so the ds_read_b128 lane groups
// (MI355X_MICROARCH.md, LDS table) need the 16-byte chunk index XORed with g(row>>2),
// g = [0,2,3,1]: checked conflict-free for all four lane groups.
// ---------------------------------------------------------------------------------------------

// ABL (ablation bits, timing experiments only; results are garbage when non-zero):
//   1 = no DMA, 2 = no fragment reads, 4 = no MFMA, 8 = no barriers
// NI = n-tiles (16 columns) per wave: 4 -> 256x256 block tile, 5 -> 256x320.  The wide flavour exists for
// the wave quantisation: N = 1280 / 3840 / 5120 at M = 32768 give 512 / 1536 / 2048 tiles = exactly
// 2 / 6 / 8 rounds over 256 CUs (256x256: 2.5 / 7.5 / 10), with 40 MFMAs per 13 fragment reads and
// 4.5 DMA pieces per wave step.  Its 20 B pieces do not divide by 8 waves: waves 0-3 (= stagger group
// 0) issue a third B piece, so the counted vmcnt waits are per group.
template <int PREC, bool OUT_F32, bool GELU, int ABL = 0, int NI = 4>
__global__ __launch_bounds__(QTHREADS) void gemm_et_big_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, void* __restrict__ Cv,
    const float* __restrict__ bias, const float* __restrict__ add2d, int add2d_period,
    int M, int N, int K, int accumulate) {
    constexpr int QBN = 64 * NI;
    constexpr int QSTAGE_ELEMS = (QBM + QBN) * QBK;                // NI = 4: 16384 ET = 32 KiB
    __shared__ __attribute__((aligned(16))) uint16_t lds[QSTAGES * QSTAGE_ELEMS];   // 128 / 144 KiB, ONE object

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;                 // waves w and w+4 share a SIMD -> different groups
    const int wm = wave >> 2, wn = wave & 3;   // wave tile rows wm*128.., cols wn*(16 NI)..

    constexpr int GROUP = 8;
    const int tiles_n = N / QBN, tiles_m = M / QBM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int per_group = GROUP * tiles_n;
    const int group = bid / per_group, first_m = group * GROUP;
    const int gsz = (tiles_m - first_m) < GROUP ? (tiles_m - first_m) : GROUP;
    const int in_g = bid - group * per_group;
    const int tile_m = first_m + in_g % gsz, tile_n = in_g / gsz;
    const int m0 = tile_m * QBM, n0 = tile_n * QBN;

    // DMA map: one piece (wave instruction) = 1 KiB = 16 rows x 64 B; lane l -> row l>>2, physical
    // chunk l&3, source chunk (l&3) ^ g(row>>2).  Round i of 8 waves covers rows 128*i + 16*w .. +15.
    const int g_row = 16 * wave + (lane >> 2);
    const int g_chunk = qswz(g_row, lane & 3);
    const uint16_t* gAg = A + (size_t)(m0 + g_row) * K + g_chunk * 8;
    const uint16_t* gBg = B + (size_t)(n0 + g_row) * K + g_chunk * 8;
    const uint32_t wave_lds_base = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds + (uint32_t)wave * (16 * QBK * 2));
    const size_t rs128 = (size_t)128 * K;
#define BIG_ISSUE(kt_, stage_)                                                                  \
    do {                                                                                         \
        const size_t koff_ = (size_t)(kt_) * QBK;                                                \
        constexpr int SB_ = (stage_) * QSTAGE_ELEMS * 2;                                         \
        glds16_asm<SB_ + 0>(gAg + koff_, wave_lds_base);                                         \
        glds16_asm<SB_ + 128 * QBK * 2>(gAg + rs128 + koff_, wave_lds_base);                     \
        glds16_asm<SB_ + QBM * QBK * 2>(gBg + koff_, wave_lds_base);                             \
        glds16_asm<SB_ + QBM * QBK * 2 + 128 * QBK * 2>(gBg + rs128 + koff_, wave_lds_base);     \
        if (NI == 5 && grp == 0)                                                                 \
            glds16_asm<SB_ + QBM * QBK * 2 + 256 * QBK * 2>(gBg + 2 * rs128 + koff_, wave_lds_base); \
    } while (0)

    f32x4_t acc[NI][8];    // [n-tile i][m-tile j]; D[i_local = n][j_local = m]
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nk = K / QBK;
    // prologue: tiles 0..2 in flight, tile 0 landed
    if (!(ABL & 1)) {
    BIG_ISSUE(0, 0);
    if (nk > 1) BIG_ISSUE(1, 1);
    if (nk > 2) BIG_ISSUE(2, 2);
    }
    // outstanding-DMA budget: this wave's pieces per tile (4, or 5 for group 0 of the wide flavour)
#define BIG_VMCNT(tiles_)                                                                        \
    do {                                                                                         \
        if (NI == 5 && grp == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((tiles_) * 5) : "memory"); \
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((tiles_) * 4) : "memory");                 \
    } while (0)
    if (nk > 2) BIG_VMCNT(2);
    else if (nk > 1) BIG_VMCNT(1);
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (grp == 1 && !(ABL & 8)) __builtin_amdgcn_s_barrier();          // stagger

    const int fr = lane & 15, fq = lane >> 4;
    // fragment byte-free offsets (elements) inside a stage; rows are fixed per lane, only the stage moves
    int offA[8], offB[NI];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const int r = wm * 128 + j * 16 + fr; offA[j] = r * QBK + qswz(r, fq) * 8; }
#pragma unroll
    for (int i = 0; i < NI; ++i) { const int r = wn * (16 * NI) + i * 16 + fr; offB[i] = QBM * QBK + r * QBK + qswz(r, fq) * 8; }

    // wait so that tile kt+1 has landed; tiles kt+2 / kt+3 may stay in flight
#define BIG_WAIT(kt_)                                                                            \
    if ((kt_) + 3 < nk) BIG_VMCNT(2);                                                            \
    else if ((kt_) + 2 < nk) BIG_VMCNT(1);                                                       \
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#define BIG_STEP(kt_, S_)                                                                        \
    if ((kt_) < nk) {                                                                            \
        uint4 fa[8], fb[NI];                                                                      \
        /* L: refill the slot freed last interval, read this step's fragments */                 \
        if (!(ABL & 1)) { if ((kt_) + 3 < nk) BIG_ISSUE((kt_) + 3, ((S_) + 3) % QSTAGES); }      \
        if (!(ABL & 2)) {                                                                        \
        _Pragma("unroll") for (int i = 0; i < NI; ++i)                                           \
            fb[i] = *reinterpret_cast<const uint4*>(lds + (S_) * QSTAGE_ELEMS + offB[i]);        \
        _Pragma("unroll") for (int j = 0; j < 8; ++j)                                            \
            fa[j] = *reinterpret_cast<const uint4*>(lds + (S_) * QSTAGE_ELEMS + offA[j]);        \
        } else {                                                                                 \
        _Pragma("unroll") for (int i = 0; i < NI; ++i) { fb[i] = make_uint4(lane, i, (kt_), 1); asm volatile("" : "+v"(fb[i].x)); } \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) { fa[j] = make_uint4(lane, j, (kt_), 2); asm volatile("" : "+v"(fa[j].x)); } \
        }                                                                                        \
        BIG_WAIT(kt_)                                                                            \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                       \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        if (!(ABL & 8)) __builtin_amdgcn_s_barrier();                                            \
        /* C: 32 MFMAs */                                                                        \
        __builtin_amdgcn_s_setprio(1);                                                           \
        if (!(ABL & 4)) {                                                                        \
        _Pragma("unroll") for (int i = 0; i < NI; ++i)                                           \
            _Pragma("unroll") for (int j = 0; j < 8; ++j)                                        \
                acc[i][j] = ET<PREC>::mfma16(fb[i], fa[j], acc[i][j]);                           \
        } else {                                                                                 \
        _Pragma("unroll") for (int i = 0; i < NI; ++i) asm volatile("" ::"v"(fb[i].x), "v"(fb[i].w)); \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) asm volatile("" ::"v"(fa[j].x), "v"(fa[j].w)); \
        }                                                                                        \
        __builtin_amdgcn_s_setprio(0);                                                           \
        BIG_WAIT(kt_)                                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        if (!(ABL & 8)) __builtin_amdgcn_s_barrier();                                            \
    }
    for (int kt = 0; kt < nk; kt += QSTAGES) {
        BIG_STEP(kt, 0)
        BIG_STEP(kt + 1, 1)
        BIG_STEP(kt + 2, 2)
        BIG_STEP(kt + 3, 3)
    }
    if (grp == 0 && !(ABL & 8)) __builtin_amdgcn_s_barrier();          // both groups: 2 + 2*nk barriers

    if (ABL & 16) {   // timing experiment: keep the accumulators alive, store nothing
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) asm volatile("" ::"v"(acc[i][j][0]), "v"(acc[i][j][3]));
        return;
    }
    {   // coalesced epilogue through the idle ring (16 KiB per wave)
        unsigned char* scr = reinterpret_cast<unsigned char*>(lds) + wave * (QSTAGES * QSTAGE_ELEMS * 2 / 8);
        const float* pre2d = OUT_F32 ? nullptr : add2d;     // ET output: the 2-D addend goes in before the rounding
        if constexpr (NI == 5 && !OUT_F32) {
            epilogue_pair_et<PREC, GELU>(acc, reinterpret_cast<unsigned char*>(lds), Cv, bias, pre2d, add2d_period, N, m0 + wm * 128,
                                         n0 + (wn >> 1) * 160, wm, wn, lane);
        } else {
            epilogue_coalesced<PREC, OUT_F32, GELU, 8, OUT_F32 ? 2 : 4, NI>(acc, scr, Cv, bias, OUT_F32 ? add2d : nullptr, add2d_period,
                                                                             N, m0 + wm * 128, n0 + wn * (16 * NI), accumulate, lane, pre2d);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// gemm_et_x64_kernel: the 256x256 / 256x320 staggered kernel re-staged in PAIR stages of 64 k.
//
// Why: the kernel above fetches a k-step of 32 ET = 64 bytes per row, i.e. HALF of a 128-byte cache line per
// row per LDS-DMA instruction, and asks for the other half one k-step (> 1 us) later, when the 32 KiB vector L1
// has long dropped the line: every line travels L2 -> L1 twice, and the per-CU L1 fill port (64 B/clk) is the
// measured ceiling of the fill path (DMA-only ablation: ~21-25 B/clk/CU useful).  Here ONE DMA
// instruction covers 8 rows x 128 bytes = 8 WHOLE lines (lanes 0-31: k-half 0, lanes 32-63: k-half 1 of the same
// rows), so each line crosses once.
//
// LDS image of a pair stage: 8-row blocks of 1 KiB = [k-half][8 rows][64 B]; inside a k-half the geometry
// (4 rows per 256-byte bank row, 16-byte chunk index XORed with g(row>>2)) is exactly the one of the kernel above,
// so its conflict-free ds_read_b128 pattern carries over unchanged.  Two pair stages = 128 / 144 KiB.
//
// Schedule (I_n = interval between consecutive block-wide raw barriers; group 1 = waves 4-7 runs one interval
// behind group 0, so that each SIMD always has one wave in its MFMA segment):
//     group 0, stage t:  I_4t   L: [issue DMA(t+1)] read fragments of k-half 0     group 1: C(t-1, half 1) [issue DMA(t+1)]
//                        I_4t+1 C: 8 NI MFMAs                                               L(t, half 0)
//                        I_4t+2 L: read fragments of k-half 1                               C(t, half 0)
//                        I_4t+3 C: 8 NI MFMAs, then vmcnt(0)                                L(t, half 1), then vmcnt(0)
// Stage t+1 goes into the buffer of stage t-1, whose last reads (group 1, I_4t-1) are complete at the barrier
// that opens I_4t; every wave retires its own pieces (vmcnt(0): one stage in flight per wave) before the barrier
// that closes I_4t+3, and the first read of stage t+1 comes after that barrier.  Each output element is accumulated
// over k in ascending 32-wide MFMA steps exactly like every other tile shape (bit-identical results).
// SPREAD: the DMA pieces are issued between the MFMAs of a C segment instead of as one burst.
// M % 256 == 0, N % (64 NI) == 0, K % 64 == 0.
// ---------------------------------------------------------------------------------------------

// Start skew of the FIRST round of blocks (experiment / tuning knob, SAMRS_GEMM_SKEW=<xcd units>,<cu-group units> in
// 1024-cycle steps): all 256 CUs start a GEMM together and reach their epilogues together, so the output tile writes
// arrive as one HBM-bound burst per round while the matrix pipes idle.  Delaying the first block of XCD x by x units (and
// CU group g by g units) keeps the rounds of different XCDs out of phase for the whole launch: one XCD writes while the
// others compute.  Blocks of later rounds inherit the skew because each CU takes its next block when it finishes one.
static int g_x64_skew = [] {
    const char* v = getenv("SAMRS_GEMM_SKEW");
    if (!v) return 0;
    int a = 0, b = 0;
    sscanf(v, "%d,%d", &a, &b);
    return (a & 0xffff) | (b << 16);
}();

// SPLIT3 (reference-grade operand split, engine option bits 16 / 32): A = A_hi + A_lo, B = B_hi + B_lo, and the product
// A_lo B_hi^T + A_hi B_lo^T + A_hi B_hi^T is ONE pass over a K axis of three segments -- the accumulators stay in registers, no
// fp32 round trip through memory between the terms (the generic route: three accumulating launches).  Pair stage st of
// 3 K / 64 reads segment st / (K / 64): the only change to the main loop is where a stage's DMA source starts.
template <bool SPLIT3>
__device__ __forceinline__ const uint16_t* seg_src_a(const uint16_t* hi, const uint16_t* lo, int st, int nst1) {
    if constexpr (!SPLIT3) return hi + (size_t)st * XBK;
    const int seg = (st >= nst1) + (st >= 2 * nst1);
    return (seg == 0 ? lo : hi) + (size_t)(st - seg * nst1) * XBK;
}
template <bool SPLIT3>
__device__ __forceinline__ const uint16_t* seg_src_b(const uint16_t* hi, const uint16_t* lo, int st, int nst1) {
    if constexpr (!SPLIT3) return hi + (size_t)st * XBK;
    const int seg = (st >= nst1) + (st >= 2 * nst1);
    return (seg == 1 ? lo : hi) + (size_t)(st - seg * nst1) * XBK;
}

// LNT (round 5): the LayerNorm that FOLLOWS this GEMM (image_encoder.py:177 norm2 after proj, :168 norm1 of the next block after
// lin2) as a tail of the GEMM itself.  The GEMM writes the fp32 residual stream in 256 x 320 tiles, a LayerNorm row needs all N = 1280
// columns = the four tiles of a 256-row panel, which four CUs of one XCD compute side by side; the stand-alone LayerNorm then re-reads
// the 168 MB stream from HBM / MALL (53 us per launch, 64 launches per encoder pass = 6 % of the step for zero FLOPs).  Here every block,
// once its own stores are complete, publishes them (agent-scope release by one lane after a block barrier: cdna_hip_programming.md
// 6 G16) and bumps a counter of its row panel; the block that finds the other tiles_n - 1 already counted -- the LAST ARRIVER -- makes
// them visible to itself (agent-scope acquire) and normalises the panel's 256 rows with layernorm_kernel's arithmetic (bit-identical
// output).  Nobody ever waits for anybody (no spin, no ordering or placement assumption: whichever block arrives last does the
// work), the counter is reset by the last arriver for the next launch.  A variant that wrote the tiles with sc1 stores instead of
// the release fence was no faster and WRONG (plain loads on another CU still hit the L2 lines the residual read had allocated).
// N <= 1280 must be the LayerNorm width.
struct LnTail {
    const float* gamma = nullptr;
    const float* beta = nullptr;
    uint16_t* out = nullptr;           // [M][N] in the operand type
    unsigned int* counters = nullptr;  // [M / 256], zero before the first launch
    float eps = 0.f;
};

// EXT (round 6, the outlier-column extension of proj / lin2: engine_state.h EncBlock::oc_*): ONE more pair stage behind the K axis whose
// 64 k come from two dense side operands A_x [M][64], B_x [N][64] (the hi + lo split of up to 32 outlier columns: A_lo | A_hi against
// B_hi | B_lo) -- the operand A is written by another kernel with its own row stride, so the extra columns cannot simply be appended
// to its rows as for qkv / lin1.  Only the DMA source of that one stage differs (row stride 64 instead of K); passed in the A_lo /
// B_lo parameters (EXT and SPLIT3 exclude each other).
template <int PREC, bool OUT_F32, bool GELU, int NI = 4, int MODE = 0, int ABL = 0, bool SPLIT3 = false, bool LNT = false, bool EXT = false>
__global__ __launch_bounds__(QTHREADS) void gemm_et_x64_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, void* __restrict__ Cv,
    const float* __restrict__ bias, const float* __restrict__ add2d, int add2d_period,
    int M, int N, int K, int accumulate, int skew,
    const uint16_t* __restrict__ A_lo = nullptr, const uint16_t* __restrict__ B_lo = nullptr, LnTail ln = LnTail()) {
    static_assert(!LNT || (OUT_F32 && !GELU), "the LayerNorm tail follows the fp32 residual outputs");
    static_assert(!(EXT && SPLIT3), "the side operands of EXT travel in the A_lo / B_lo parameters");
    constexpr int XBN = 64 * NI;
    constexpr int XROWS = QBM + XBN;                       // 512 / 576 rows per stage
    constexpr int XSTAGE_ELEMS = XROWS * XBK;              // 64 / 72 KiB
    constexpr uint32_t XSB = XSTAGE_ELEMS * 2;             // stage bytes
    constexpr int NPIECE = 4 + NI;                         // DMA pieces per wave and stage (8 rows x 128 B each): 4 A + NI B
    constexpr bool SPREAD = (MODE & 1) != 0;               // DMA pieces issued between the MFMAs instead of as one burst
    // LIGHT: ONE block-wide barrier per pair stage (the one that hands a landed stage over) instead of four.  The
    // barriers between the L and C segments of a stage guard no LDS hazard -- they only keep the two waves of a
    // SIMD in complementary segments, at ~150 cycles of re-convergence per 640-cycle MFMA segment.  Without them
    // group 1 still runs half a stage behind group 0 (its rendezvous sits between L(t, 1) and C(t, 1)), so its
    // fragment reads fall into the other wave's MFMA segments by themselves.
    constexpr bool LIGHT = (MODE & 2) != 0;
    constexpr bool NOPRIO = (MODE & 4) != 0;               // experiment: no s_setprio around the MFMA segments
    // ABL (timing experiments only, results are garbage): 1 no DMA, 2 no fragment reads, 4 no MFMA, 16 no epilogue
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * XSTAGE_ELEMS];   // 128 / 144 KiB, ONE object

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;                 // waves w and w+4 share a SIMD -> different groups
    const int wm = wave >> 2, wn = wave & 3;   // wave tile rows wm*128.., cols wn*(16 NI)..

    constexpr int GROUP = 8;
    const int tiles_n = N / XBN, tiles_m = M / QBM;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int per_group = GROUP * tiles_n;
    const int group = bid / per_group, first_m = group * GROUP;
    const int gsz = (tiles_m - first_m) < GROUP ? (tiles_m - first_m) : GROUP;
    const int in_g = bid - group * per_group;
    const int tile_m = first_m + in_g % gsz, tile_n = in_g / gsz;
    const int m0 = tile_m * QBM, n0 = tile_n * XBN;

    // DMA map: piece q of this wave covers stage rows 64 q + 8 wave .. + 7 (q < 4: A rows, else B rows 64 (q - 4) + ..);
    // lane l -> k-half l>>5, row (l>>2)&7, physical chunk l&3 which holds source chunk (l&3) ^ g(row>>2) (g depends on
    // row mod 16 only, and 64 q = 0 mod 16).  The per-lane byte offset is the same for A and B (both have row stride K).
    const int prow = 8 * wave + ((lane >> 2) & 7);
    const uint32_t voff = ((uint32_t)prow * (uint32_t)K + (uint32_t)(lane >> 5) * 32u + (uint32_t)qswz(prow, lane & 3) * 8u) * 2u;
    const uint16_t* sA = A + (size_t)m0 * K;               // wave-uniform bases (SGPR pairs)
    const uint16_t* sB = B + (size_t)n0 * K;
    const uint16_t* sAl = SPLIT3 ? A_lo + (size_t)m0 * K : nullptr;
    const uint16_t* sBl = SPLIT3 ? B_lo + (size_t)n0 * K : nullptr;
    const int nst1 = K / XBK;                              // pair stages per K segment
    const size_t rs64 = (size_t)64 * K;
    // EXT: the side operands' tile bases and the per-lane offset on their 64-element rows
    const uint16_t* sAx = EXT ? A_lo + (size_t)m0 * XBK : nullptr;
    const uint16_t* sBx = EXT ? B_lo + (size_t)n0 * XBK : nullptr;
    const uint32_t voffx = ((uint32_t)prow * (uint32_t)XBK + (uint32_t)(lane >> 5) * 32u + (uint32_t)qswz(prow, lane & 3) * 8u) * 2u;
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds + (uint32_t)wave * 1024u);
    // piece q_ (literal) of pair stage st_ into the buffer at byte offset wr_
    // EXT: where the pieces of a stage come from is chosen ONCE per stage (X64_SEL: wave-uniform selects into xpa / xpb / xprs and one
    // v_cndmask for the lane offset), not by a branch in front of each of its nine pieces inside the MFMA stream (the first form: lin2
    // + 17 us for 1 / 80 more work).  The other instantiations never see these variables.
    const uint16_t *xpa = sA, *xpb = sB;
    size_t xprs = rs64;
    uint32_t xvo = voff;
#define X64_SEL(st_)                                                                                       \
    if constexpr (EXT) {                                                                                   \
        const bool xs_ = (st_) == nst1;                                                                    \
        xpa = xs_ ? sAx : sA + (size_t)(st_) * XBK;                                                        \
        xpb = xs_ ? sBx : sB + (size_t)(st_) * XBK;                                                        \
        xprs = xs_ ? (size_t)(64 * XBK) : rs64;                                                            \
        xvo = xs_ ? voffx : voff;                                                                          \
    }
#define X64_PIECE(st_, wr_, q_)                                                                            \
    if constexpr (!(ABL & 1)) {                                                                            \
        if constexpr (EXT)                                                                                 \
            glds16_s(xvo, ((q_) < 4 ? xpa + (size_t)(q_) * xprs : xpb + (size_t)((q_) - 4) * xprs),                                      \
                     lds0 + (wr_) + ((q_) < 4 ? (q_) * 8192u : (uint32_t)(QBM * XBK * 2) + ((q_) - 4) * 8192u));                         \
        else                                                                                               \
            glds16_s(voff, ((q_) < 4 ? seg_src_a<SPLIT3>(sA, sAl, (st_), nst1) + (size_t)(q_) * rs64                                    \
                                      : seg_src_b<SPLIT3>(sB, sBl, (st_), nst1) + (size_t)((q_) - 4) * rs64),                            \
                     lds0 + (wr_) + ((q_) < 4 ? (q_) * 8192u : (uint32_t)(QBM * XBK * 2) + ((q_) - 4) * 8192u));                         \
    }
#define X64_ISSUE(st_, wr_)                                                                                \
    do {                                                                                                   \
        X64_SEL(st_)                                                                                       \
        X64_PIECE(st_, wr_, 0); X64_PIECE(st_, wr_, 1); X64_PIECE(st_, wr_, 2); X64_PIECE(st_, wr_, 3);    \
        X64_PIECE(st_, wr_, 4); X64_PIECE(st_, wr_, 5); X64_PIECE(st_, wr_, 6); X64_PIECE(st_, wr_, 7);    \
        if constexpr (NPIECE == 9) X64_PIECE(st_, wr_, 8);                                                 \
    } while (0)

    f32x4_t acc[NI][8];    // [n-tile i][m-tile j]
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nst = (SPLIT3 ? 3 : 1) * nst1 + (EXT ? 1 : 0);
    const int fr = lane & 15, fq = lane >> 4;
    // fragment BYTE offsets inside a stage for k-half 0; k-half 1 is +512
    uint32_t offA[8], offB[NI];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const int r = wm * 128 + j * 16 + fr; offA[j] = ((r >> 3) * 512 + (r & 7) * 32 + qswz(r, fq) * 8) * 2; }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int r = QBM + wn * (16 * NI) + i * 16 + fr;
        offB[i] = ((r >> 3) * 512 + (r & 7) * 32 + qswz(r, fq) * 8) * 2;
    }
    const unsigned char* ldsb = reinterpret_cast<const unsigned char*>(lds);

    // ABL 64 (timing experiment): wave 0 records s_memtime stamps into the buffer passed as add2d: 32 x u64 per block
    // [0] entry, [1] stage 0 landed, [2 + t] end of stage t (t < 24), [26] loop done, [27] epilogue done, [28] HW_ID | XCC_ID << 32
    unsigned long long* tl = nullptr;
    if constexpr (ABL & 64) {
        tl = reinterpret_cast<unsigned long long*>(const_cast<float*>(add2d)) + (size_t)blockIdx.x * 32;
        if (tid == 0) {
            tl[0] = __builtin_amdgcn_s_memtime();
            tl[28] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) |
                     ((unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20) << 32);
        }
    }
    if (skew && blockIdx.x < 256) {            // first round only (one block per CU; block b starts on XCD b % 8)
        const int n = (int)(blockIdx.x & 7) * (skew & 0xffff) + (int)((blockIdx.x >> 3) & 3) * (skew >> 16);
        for (int i = 0; i < n; ++i) __builtin_amdgcn_s_sleep(16);      // 16 x 64 cycles
    }
    // prologue: stage 0 landed for everybody
    X64_ISSUE(0, 0u);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if constexpr (ABL & 64) { if (tid == 0) tl[1] = __builtin_amdgcn_s_memtime(); }
    if (grp == 1) {                            // I_0 of group 1: nothing to compute yet; its share of stage 1 goes out
        if (nst > 1) X64_ISSUE(1, XSB);
        __builtin_amdgcn_s_barrier();
    }

#define X64_READ(rd_, kh_)                                                                                 \
    if constexpr (!(ABL & 2)) {                                                                            \
    _Pragma("unroll") for (int i = 0; i < NI; ++i)                                                         \
        fb[i] = *reinterpret_cast<const uint4*>(ldsb + (rd_) + (kh_) * 512 + offB[i]);                     \
    _Pragma("unroll") for (int j = 0; j < 8; ++j)                                                          \
        fa[j] = *reinterpret_cast<const uint4*>(ldsb + (rd_) + (kh_) * 512 + offA[j]);                     \
    } else {                                                                                               \
    _Pragma("unroll") for (int i = 0; i < NI; ++i) { fb[i] = make_uint4(lane, i, (rd_), 1); asm volatile("" : "+v"(fb[i].x)); } \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) { fa[j] = make_uint4(lane, j, (rd_), 2); asm volatile("" : "+v"(fa[j].x)); } \
    }
    // 8 NI MFMAs of one k-half; when dma_ (wave-uniform) is set, this wave's pieces of stage st_ go out first (burst)
    // or one per m-tile row of MFMAs (SPREAD).  The accumulators never sit inside a conditional region.
#define X64_MFMA(dma_, st_, wr_)                                                                           \
    if (!SPREAD) { if (dma_) X64_ISSUE(st_, wr_); }                                                        \
    if (SPREAD) { X64_SEL(st_) }                                                                           \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                        \
        if constexpr (!(ABL & 4)) {                                                                        \
        _Pragma("unroll") for (int i = 0; i < NI; ++i) acc[i][j] = ET<PREC>::mfma16(fb[i], fa[j], acc[i][j]); \
        } else {                                                                                           \
        _Pragma("unroll") for (int i = 0; i < NI; ++i) asm volatile("" ::"v"(fb[i].x), "v"(fb[i].w), "v"(fa[j].x), "v"(fa[j].w)); \
        }                                                                                                  \
        if (SPREAD) {                                                                                      \
            if (dma_) {                                                                                    \
                if (j == 0) X64_PIECE(st_, wr_, 0); if (j == 1) X64_PIECE(st_, wr_, 1);                    \
                if (j == 2) X64_PIECE(st_, wr_, 2); if (j == 3) X64_PIECE(st_, wr_, 3);                    \
                if (j == 4) X64_PIECE(st_, wr_, 4); if (j == 5) X64_PIECE(st_, wr_, 5);                    \
                if (j == 6) X64_PIECE(st_, wr_, 6);                                                        \
                if (j == 7) { X64_PIECE(st_, wr_, 7); if constexpr (NPIECE == 9) X64_PIECE(st_, wr_, 8); } \
            }                                                                                              \
        }                                                                                                  \
    }
    // intra-stage barrier (kept only in the four-barrier schedule)
#define X64_MIDBAR() if constexpr (!LIGHT) __builtin_amdgcn_s_barrier();

    uint32_t rd = 0;                           // byte offset of the buffer that holds stage t
    for (int t = 0; t < nst; ++t) {
        uint4 fa[8], fb[NI];
        const uint32_t wr = XSB - rd;
        const bool dma0 = (grp == 0) && (t + 1 < nst);     // group 0 feeds stage t+1 from I_4t
        const bool dma1 = (grp == 1) && (t + 2 < nst);     // group 1 feeds stage t+2 from its C(t, 1) = I_4(t+1)
        // LIGHT: rendezvous R_t -- group 0 arrives here (stage t-1 finished, its pieces of stage t landed), group 1
        // from between L(t-1, 1) and C(t-1, 1) (t = 0: from the prologue)
        if constexpr (LIGHT) { if (grp == 0) __builtin_amdgcn_s_barrier(); }
        // ---- L(t, 0) ----
        if (!SPREAD) { if (dma0) X64_ISSUE(t + 1, wr); }
        X64_READ(rd, 0)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        X64_MIDBAR()
        // ---- C(t, 0) ----
        if constexpr (!NOPRIO) __builtin_amdgcn_s_setprio(1);
        X64_MFMA(SPREAD && dma0, t + 1, wr)
        if constexpr (!NOPRIO) __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        X64_MIDBAR()
        // ---- L(t, 1); group 1: its pieces of stage t+1 (issued one stage ago) must have landed ----
        X64_READ(rd, 1)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (grp == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (LIGHT) { if (grp == 1) __builtin_amdgcn_s_barrier(); } else __builtin_amdgcn_s_barrier();
        // ---- C(t, 1); group 1: buffer `rd` is free from here on (both groups have read k-half 1) ----
        if constexpr (!NOPRIO) __builtin_amdgcn_s_setprio(1);
        X64_MFMA(dma1, t + 2, rd)
        if constexpr (!NOPRIO) __builtin_amdgcn_s_setprio(0);
        if (grp == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (!LIGHT) __builtin_amdgcn_s_barrier();
        if constexpr (ABL & 64) { if (tid == 0 && t < 24) tl[2 + t] = __builtin_amdgcn_s_memtime(); }
        rd = wr;
    }
    if (grp == 0) __builtin_amdgcn_s_barrier();          // both groups: same barrier count; every ring read is done

    if constexpr (ABL & 64) { if (tid == 0) tl[26] = __builtin_amdgcn_s_memtime(); }
    if constexpr (ABL & 16) {   // timing experiment: keep the accumulators alive, store nothing
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) asm volatile("" ::"v"(acc[i][j][0]), "v"(acc[i][j][3]));
        return;
    }
    {   // coalesced epilogue through the idle ring (16 / 18 KiB per wave), identical to the kernel above
        unsigned char* scr = reinterpret_cast<unsigned char*>(lds) + wave * (2 * XSB / 8);
        const float* pre2d = OUT_F32 ? nullptr : add2d;     // ET output: the 2-D addend goes in before the rounding
        // ABL 32 (timing experiment): every block stores to the SAME 256 x 64 NI window -> the stores stay in the L2
        const int em0 = (ABL & 32) ? 0 : m0, en0 = (ABL & 32) ? 0 : n0;
        if constexpr (NI == 5 && !OUT_F32) {
            epilogue_pair_et<PREC, GELU>(acc, reinterpret_cast<unsigned char*>(lds), Cv, bias, pre2d, add2d_period, N, em0 + wm * 128,
                                         en0 + (wn >> 1) * 160, wm, wn, lane);
        } else {
            epilogue_coalesced<PREC, OUT_F32, GELU, 8, OUT_F32 ? 2 : 4, NI>(acc, scr, Cv, bias, OUT_F32 ? add2d : nullptr, add2d_period,
                                                                             N, em0 + wm * 128, en0 + wn * (16 * NI), accumulate, lane, pre2d);
        }
    }
    if constexpr (ABL & 64) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // stores acknowledged: what s_endpgm would wait for anyway
        if (tid == 0) tl[27] = __builtin_amdgcn_s_memtime();
    }
    if constexpr (LNT) {
        int* flag = reinterpret_cast<int*>(lds);               // the ring is idle: every wave is past its bounce after the barrier below
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's stores of the tile have completed
        __syncthreads();                                       // ... everybody's
        if (threadIdx.x == 0) {
            // publish the tile (agent-scope release: L2 write-back), count it, and if it was the panel's last: make the other
            // tiles visible to this CU (agent-scope acquire).  cdna_hip_programming.md 6 G16: placement-independent.
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            const unsigned int old = __hip_atomic_fetch_add(ln.counters + tile_m, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = old == (unsigned int)(tiles_n - 1);
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                __hip_atomic_store(ln.counters + tile_m, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // ready for the next launch
            }
            *flag = last;
        }
        __syncthreads();
        if (*flag == 0) return;
        // ---- last arriver: LayerNorm of rows m0 .. m0 + 255: wave w takes rows 32 w .. 32 w + 31, one row at a time with
        // layernorm_kernel's arithmetic, the next row's loads in flight under the current row's.  Everything the tail needs is
        // RE-DERIVED here from an opaque copy of threadIdx.x: the kernel sits at 256 VGPRs, and every value kept alive across the
        // epilogue for the tail's sake turned into scratch traffic inside the epilogue of EVERY block (versions 1 - 3: forty spill
        // instructions there, each with a vmcnt(0) that serialises the residual loads: +185 us per launch, profiles/r05_ln_tail.txt).
        int tid_t = threadIdx.x;
        asm volatile("" : "+v"(tid_t));
        const int lane_t = tid_t & 63, wave_t = __builtin_amdgcn_readfirstlane(tid_t >> 6);
        // Latency: by the time the last tile lands most of the panel has left the 4 MB L2 (a round of tiles writes 10 MB per XCD), a
        // row costs a ~3 us trip to the Infinity Cache / HBM, and with ONE row in flight per wave the tail took 100 us (version 4:
        // proj + tail 340 us against 134 + 53, rocprofv3).  So a ring of eight row buffers per wave: 64 rows = 320 KB in flight per CU.
        constexpr int LNV = 5, LNP = 8;                        // float4 per lane and row (N <= 1280); rows in flight per wave
        const int nv = N >> 2;
        const float* X = reinterpret_cast<const float*>(Cv);
        float4 ring[LNP][LNV];
        const int row0 = tile_m * QBM + wave_t * 32;
#define LNT_LOAD(slot_, row_)                                                                              \
        {                                                                                                  \
            const float4* xr_ = reinterpret_cast<const float4*>(X + (size_t)(row_) * N);                    \
            _Pragma("unroll") for (int i = 0; i < LNV; ++i) { const int idx = lane_t + 64 * i; if (idx < nv) ring[slot_][i] = xr_[idx]; } \
        }
#pragma unroll
        for (int sl = 0; sl < LNP; ++sl) LNT_LOAD(sl, row0 + sl)
        for (int g = 0; g < 32 / LNP; ++g) {
#pragma unroll
            for (int sl = 0; sl < LNP; ++sl) {
                const int row = row0 + g * LNP + sl;
                float sm = 0.f;
#pragma unroll
                for (int i = 0; i < LNV; ++i) {
                    const int idx = lane_t + 64 * i;
                    if (idx < nv) sm += (ring[sl][i].x + ring[sl][i].y) + (ring[sl][i].z + ring[sl][i].w);
                }
                const float mean = wave_sum(sm) / (float)N;
                float q = 0.f;
#pragma unroll
                for (int i = 0; i < LNV; ++i) {
                    const int idx = lane_t + 64 * i;
                    if (idx < nv) {
                        const float a = ring[sl][i].x - mean, b = ring[sl][i].y - mean, c = ring[sl][i].z - mean, d = ring[sl][i].w - mean;
                        q += (a * a + b * b) + (c * c + d * d);
                    }
                }
                const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)N + ln.eps);
#pragma unroll
                for (int i = 0; i < LNV; ++i) {
                    const int idx = lane_t + 64 * i;
                    if (idx < nv) {
                        const float4 g4 = reinterpret_cast<const float4*>(ln.gamma)[idx];
                        const float4 bt = reinterpret_cast<const float4*>(ln.beta)[idx];
                        const float o0 = (ring[sl][i].x - mean) * rstd * g4.x + bt.x;
                        const float o1 = (ring[sl][i].y - mean) * rstd * g4.y + bt.y;
                        const float o2 = (ring[sl][i].z - mean) * rstd * g4.z + bt.z;
                        const float o3 = (ring[sl][i].w - mean) * rstd * g4.w + bt.w;
                        uint2 o;
                        o.x = pack2<PREC>(o0, o1);
                        o.y = pack2<PREC>(o2, o3);
                        reinterpret_cast<uint2*>(ln.out + (size_t)row * N)[idx] = o;
                    }
                }
                if (g + 1 < 32 / LNP) LNT_LOAD(sl, row + LNP)       // this slot's next row goes out as soon as the slot is free
            }
        }
#undef LNT_LOAD
    }
#undef X64_PIECE
#undef X64_SEL
#undef X64_ISSUE
#undef X64_READ
#undef X64_MFMA
#undef X64_MIDBAR
}

// ---------------------------------------------------------------------------------------------
// gemm_et_x64p_kernel: the pair-stage 256x320 kernel (one barrier per stage, spread DMA) made PERSISTENT: one block per
// CU walks tiles L, L + gridDim.x, ...  Measured on the one-tile-per-block kernel (s_memtime stamps, tools/gemm_timeline.py,
// qkv shape): of ~90 k cycles per tile, 3.2 k pass before stage 0 has landed, 2.3 k between a block's end and its successor's
// first instruction, and the block's last ~2 k wait for store acknowledgements.  Here the next tile's stage 0 goes out
// (into ring buffer 0, free since the last rendezvous) BEFORE the epilogue, whose bounce scratch is confined to ring buffer
// 1; every wave retires those pieces just before its first store (epilogue DRAIN), so the stores are never waited for: the
// next tile's main loop starts right after the epilogue, with its stage 0 already in LDS.  Main loop = the kernel above.
// add2d is not supported (the encoder's four big GEMMs have none).
// ---------------------------------------------------------------------------------------------
//
// FOLD: the LayerNorm in front of this GEMM (image_encoder.py:168,177) folded into it.  A = the raw residual stream rounded to
// ET (written by the GEMM that produced it, gemm_et_m32_kernel<STATS>), B = W diag(gamma) rounded to ET, cvec_n = sum_k of
// that B row, bias_n = b_n + sum_k W_nk beta_k:
//     LN(x) W^T + b  =  rstd (x W'^T - mean cvec) + bias'
// rowstat[m] = (rstd, -rstd mean) comes from ln_rowstat_kernel (encoder_kernels.hip), which merges the per-row (mean, M2)
// partials of the LN_NS 160-column groups; only the ET epilogue reads it (8 bytes per row and lane, next to the bias loads).

// MXO (round 4; ET output, no FOLD / SPLIT3): the epilogue also writes the output as MXFP4 hi / lo rows (epilogue_pair_et<MXO>: lin1 of
// split 207, whose lin2 takes MXFP4 lo terms while lin1 itself takes none).  The four output pointers travel in their own MxOut
// parameter (round 5: they used to be smuggled through rowstat / cvec / A_lo / B_lo with const_casts); the flavours that do not
// use it never load it from the kernarg segment, so their code is what it was.
template <int PREC, bool OUT_F32, int GELU /* 0 none, 1 fp32-epsilon erf, 2 the 1x-rate mode's cheaper erf (ET output only) */, bool FOLD = false,
          bool SPLIT3 = false, bool MXO = false, bool STREAM = false /* plain ET flavours: non-temporal output stores (stream_hidden) */>
__global__ __launch_bounds__(QTHREADS) void gemm_et_x64p_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, void* __restrict__ Cv,
    const float* __restrict__ bias, int M, int N, int K, int accumulate,
    const float2* __restrict__ rowstat = nullptr, const float* __restrict__ cvec = nullptr,
    const uint16_t* __restrict__ A_lo = nullptr, const uint16_t* __restrict__ B_lo = nullptr, int split_from_n = 0,
    MxOut mxo = MxOut(), int ld = 0 /* row stride of A and B in elements, 0 = K (gemm_ld_ok: operands padded off the 2560-byte stride) */) {
    static_assert(!(FOLD && OUT_F32), "the folded LayerNorm feeds ET outputs only (qkv, lin1)");
    static_assert(!(FOLD && SPLIT3), "the split operands come from an explicit LayerNorm");
    static_assert(!(MXO && (FOLD || SPLIT3 || OUT_F32)), "MX rows go with the plain ET-output flavour");
    constexpr int NI = 5;
    constexpr int XBN = 64 * NI;
    constexpr int XROWS = QBM + XBN;
    constexpr int XSTAGE_ELEMS = XROWS * XBK;
    constexpr uint32_t XSB = XSTAGE_ELEMS * 2;
    constexpr int NPIECE = 4 + NI;
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * XSTAGE_ELEMS];   // 144 KiB, ONE object

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;
    const int wm = wave >> 2, wn = wave & 3;

    constexpr int GROUP = 8;
    const int tiles_n = N / XBN, tiles_m = M / QBM, ntiles = tiles_n * tiles_m;
    const int per_group = GROUP * tiles_n;
#define X64P_TILE(L_, m_, n_)                                                                    \
    do {                                                                                         \
        const int bid_ = xcd_remap((L_), ntiles);                                                \
        const int group_ = bid_ / per_group, first_m_ = group_ * GROUP;                           \
        const int gsz_ = (tiles_m - first_m_) < GROUP ? (tiles_m - first_m_) : GROUP;            \
        const int in_g_ = bid_ - group_ * per_group;                                             \
        (m_) = (first_m_ + in_g_ % gsz_) * QBM;                                                  \
        (n_) = (in_g_ / gsz_) * XBN;                                                             \
    } while (0)

    const int LD = ld > 0 ? ld : K;                // operand row stride (elements)
    const int prow = 8 * wave + ((lane >> 2) & 7);
    const uint32_t voff = ((uint32_t)prow * (uint32_t)LD + (uint32_t)(lane >> 5) * 32u + (uint32_t)qswz(prow, lane & 3) * 8u) * 2u;
    const size_t rs64 = (size_t)64 * LD;
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds + (uint32_t)wave * 1024u);
    const uint16_t* sA;                            // wave-uniform bases of the tile being FED (SGPR pairs)
    const uint16_t* sB;
    const uint16_t* sAl = nullptr;                 // SPLIT3: the lo operands of that tile
    const uint16_t* sBl = nullptr;
    const int nst1 = K / XBK;                      // pair stages per K segment
    // SPLIT3 with split_from_n > 0: only output columns >= split_from_n take the lo terms (qkv: the v third -- q and k pass
    // through the softmax, error_budget.py plans4); the other tiles start at the hi x hi segment: stage base sb = 2 nst1
    int sb = 0;                                    // of the tile being FED
#define X64P_PIECE(st_, wr_, q_)                                                                           \
    glds16_s(voff, ((q_) < 4 ? seg_src_a<SPLIT3>(sA, sAl, (st_) + sb, nst1) + (size_t)(q_) * rs64          \
                             : seg_src_b<SPLIT3>(sB, sBl, (st_) + sb, nst1) + (size_t)((q_) - 4) * rs64),  \
             lds0 + (wr_) + ((q_) < 4 ? (q_) * 8192u : (uint32_t)(QBM * XBK * 2) + ((q_) - 4) * 8192u))
#define X64P_ISSUE(st_, wr_)                                                                               \
    do {                                                                                                   \
        X64P_PIECE(st_, wr_, 0); X64P_PIECE(st_, wr_, 1); X64P_PIECE(st_, wr_, 2); X64P_PIECE(st_, wr_, 3); \
        X64P_PIECE(st_, wr_, 4); X64P_PIECE(st_, wr_, 5); X64P_PIECE(st_, wr_, 6); X64P_PIECE(st_, wr_, 7); \
        X64P_PIECE(st_, wr_, 8);                                                                           \
    } while (0)

    const int fr = lane & 15, fq = lane >> 4;
    uint32_t offA[8], offB[NI];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const int r = wm * 128 + j * 16 + fr; offA[j] = ((r >> 3) * 512 + (r & 7) * 32 + qswz(r, fq) * 8) * 2; }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int r = QBM + wn * (16 * NI) + i * 16 + fr;
        offB[i] = ((r >> 3) * 512 + (r & 7) * 32 + qswz(r, fq) * 8) * 2;
    }
    const unsigned char* ldsb = reinterpret_cast<const unsigned char*>(lds);

#define X64P_READ(rd_, kh_)                                                                                \
    _Pragma("unroll") for (int i = 0; i < NI; ++i)                                                         \
        fb[i] = *reinterpret_cast<const uint4*>(ldsb + (rd_) + (kh_) * 512 + offB[i]);                     \
    _Pragma("unroll") for (int j = 0; j < 8; ++j)                                                          \
        fa[j] = *reinterpret_cast<const uint4*>(ldsb + (rd_) + (kh_) * 512 + offA[j]);
#define X64P_MFMA(dma_, st_, wr_)                                                                          \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                        \
        _Pragma("unroll") for (int i = 0; i < NI; ++i) acc[i][j] = ET<PREC>::mfma16(fb[i], fa[j], acc[i][j]); \
        if (dma_) {                                                                                        \
            if (j == 0) X64P_PIECE(st_, wr_, 0); if (j == 1) X64P_PIECE(st_, wr_, 1);                      \
            if (j == 2) X64P_PIECE(st_, wr_, 2); if (j == 3) X64P_PIECE(st_, wr_, 3);                      \
            if (j == 4) X64P_PIECE(st_, wr_, 4); if (j == 5) X64P_PIECE(st_, wr_, 5);                      \
            if (j == 6) X64P_PIECE(st_, wr_, 6);                                                           \
            if (j == 7) { X64P_PIECE(st_, wr_, 7); X64P_PIECE(st_, wr_, 8); }                              \
        }                                                                                                  \
    }

    int L = blockIdx.x, m0, n0;
    X64P_TILE(L, m0, n0);
    sA = A + (size_t)m0 * LD;
    sB = B + (size_t)n0 * LD;
    if constexpr (SPLIT3) { sAl = A_lo + (size_t)m0 * LD; sBl = B_lo + (size_t)n0 * LD; sb = n0 >= split_from_n ? 0 : 2 * nst1; }
    X64P_ISSUE(0, 0u);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    f32x4_t acc[NI][8];
    for (;;) {
        const int nst = SPLIT3 ? 3 * nst1 - sb : nst1;       // stages of THIS tile (sb still is its base here)
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (grp == 1) {                        // rendezvous R_0 of group 1; its share of stage 1 goes out first
            if (nst > 1) X64P_ISSUE(1, XSB);
            __builtin_amdgcn_s_barrier();
        }
        uint32_t rd = 0;
        for (int t = 0; t < nst; ++t) {
            uint4 fa[8], fb[NI];
            const uint32_t wr = XSB - rd;
            const bool dma0 = (grp == 0) && (t + 1 < nst);
            const bool dma1 = (grp == 1) && (t + 2 < nst);
            if (grp == 0) __builtin_amdgcn_s_barrier();                       // R_t
            X64P_READ(rd, 0)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_setprio(1);
            X64P_MFMA(dma0, t + 1, wr)
            __builtin_amdgcn_s_setprio(0);
            __builtin_amdgcn_sched_barrier(0);
            X64P_READ(rd, 1)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (grp == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            if (grp == 1) __builtin_amdgcn_s_barrier();                       // R_{t+1} of group 1
            __builtin_amdgcn_s_setprio(1);
            X64P_MFMA(dma1, t + 2, rd)
            __builtin_amdgcn_s_setprio(0);
            if (grp == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            rd = wr;
        }
        if (grp == 0) __builtin_amdgcn_s_barrier();      // last rendezvous: every ring read of this tile is done

        // next tile: its stage 0 goes into ring buffer 0 now and lands under the epilogue
        const int Ln = L + (int)gridDim.x;
        const bool more = Ln < ntiles;
        int m1 = m0, n1 = n0;
        if (more) {
            X64P_TILE(Ln, m1, n1);
            sA = A + (size_t)m1 * LD;
            sB = B + (size_t)n1 * LD;
            if constexpr (SPLIT3) { sAl = A_lo + (size_t)m1 * LD; sBl = B_lo + (size_t)n1 * LD; sb = n1 >= split_from_n ? 0 : 2 * nst1; }
            X64P_ISSUE(0, 0u);
        }
        {   // epilogue of tile (m0, n0); bounce scratch = ring buffer 1 only (72 KiB: 9 KiB per wave / 18 KiB per pair)
            unsigned char* upper = reinterpret_cast<unsigned char*>(lds) + XSB;
            if constexpr (MXO) {
                epilogue_pair_et<PREC, GELU, 2, true, false, true>(acc, upper, Cv, bias, nullptr, 1, N, m0 + wm * 128, n0 + (wn >> 1) * 160, wm, wn,
                                                                   lane, nullptr, nullptr, mxo);
            } else if constexpr (!OUT_F32) {
                epilogue_pair_et<PREC, GELU, 2, true, FOLD, false, STREAM>(acc, upper, Cv, bias, nullptr, 1, N, m0 + wm * 128, n0 + (wn >> 1) * 160, wm, wn,
                                                                           lane, rowstat, cvec);
            } else {
                epilogue_coalesced<PREC, true, GELU != 0, 8, 1, NI, false, true>(acc, upper + wave * (XSB / 8), Cv, bias, nullptr, 1, N,
                                                                           m0 + wm * 128, n0 + wn * (16 * NI), accumulate, lane);
            }
        }
        if (!more) break;
        __builtin_amdgcn_s_barrier();          // scratch free again; stage 0 visible (each wave drained its pieces before its first store)
        L = Ln; m0 = m1; n0 = n1;
    }
#undef X64P_TILE
#undef X64P_PIECE
#undef X64P_ISSUE
#undef X64P_READ
#undef X64P_MFMA
}

// gelu_form (GemmOpts): erf form of the ET-output GELU epilogue of the persistent kernels (lin1 of ViT-H): 1 = fp32-epsilon class
// (A-S 7.1.26), 2 = the cheaper one (A-S 7.1.28, common.h gelu_erf2_et)
// ld (GemmOpts): row stride (elements) of the A and B operands of a plain ET launch, 0 = K.  Round 5, late: at K = 1280 an
// operand row is 2560 B = ten 256-byte units, so the 256 rows a tile fetches per k-slice fall on half of the memory channels; stored with a
// stride of 1408 elements (eleven units: every channel) the same kernels run their main loops ~4 % faster (tools/gemm_bench.py STRIDE_PROBE:
// lin1 + GELU 432.2 us at K = 1280, 451.5 at K = 1408 with 10 % more stages).  Only the persistent ET kernels take a stride (gemm_ld_ok says
// whether a launch will run on one of them); the engine pads the LayerNorm output and keeps padded copies of the qkv / lin1 weights.
// lin1's output -- the MLP hidden tensor, read once, by lin2 -- is written with NON-TEMPORAL stores when it is larger than the 256 MB
// Infinity Cache it would otherwise be allocated in (8 tiles of ViT-H: 336 MB per launch; SAMRS_NT_HIDDEN=0 / 1 forces the choice).
// Measured on MI355X, libraries alternated on one box (profiles/r05_nt_streams.txt): lin1 424 -> 408 us in situ (the write-allocates no
// longer push the A / B panels out of the L2s), lin2 / proj -7 us on average (the residual stream survives longer), the 8-tile step
// +1.1 ... +1.4 % on three boxes.  The same hint on q | k | v, the LayerNorm or the attention output LOSES 2 - 3.5 % (their consumers live
// on finding them cached), and on lin2's A-row loads it gives the gain back (four tile columns re-read those rows from the L2).
static bool stream_hidden(long M, long N) {
    static const int mode = [] { const char* v = getenv("SAMRS_NT_HIDDEN"); return v ? atoi(v) : -1; }();
    if (mode >= 0) return mode != 0;
    return M * N * 2 >= (256L << 20);
}
template <int PREC>
hipError_t launch_gemm_x64p(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, bool out_f32, bool gelu,
                            bool accumulate, int ld, int gelu_form, hipStream_t s) {
    const int ntiles = (M / QBM) * (N / WBN);
    const int n_cu = cu_count();
    dim3 grid(ntiles < n_cu ? ntiles : n_cu), block(QTHREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    const int acc = accumulate ? 1 : 0;
    if (out_f32) {
        if (gelu) gemm_et_x64p_kernel<PREC, true, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc);
        else gemm_et_x64p_kernel<PREC, true, false><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc);
    } else {
        const bool so = gelu && stream_hidden(M, N);
#define X64P_ARGS a, b, C, bias, M, N, K, acc, nullptr, nullptr, nullptr, nullptr, 0, MxOut(), ld
        if (gelu && gelu_form == 2 && so) gemm_et_x64p_kernel<PREC, false, 2, false, false, false, true><<<grid, block, 0, s>>>(X64P_ARGS);
        else if (gelu && gelu_form == 2) gemm_et_x64p_kernel<PREC, false, 2><<<grid, block, 0, s>>>(X64P_ARGS);
        else if (gelu && so) gemm_et_x64p_kernel<PREC, false, true, false, false, false, true><<<grid, block, 0, s>>>(X64P_ARGS);
        else if (gelu) gemm_et_x64p_kernel<PREC, false, true><<<grid, block, 0, s>>>(X64P_ARGS);
        else gemm_et_x64p_kernel<PREC, false, false><<<grid, block, 0, s>>>(X64P_ARGS);
#undef X64P_ARGS
    }
    return hipGetLastError();
}

// ET output (+ GELU) that is also written as MXFP4 hi / lo rows: the persistent kernel with the MX-row epilogue, no lo terms taken
template <int PREC>
hipError_t launch_gemm_x64p_mxo(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, bool gelu,
                                void* o4_hi, void* o4_lo, void* so_hi, void* so_lo, hipStream_t s) {
    const int ntiles = (M / QBM) * (N / WBN);
    const int n_cu = cu_count();
    dim3 grid(ntiles < n_cu ? ntiles : n_cu), block(QTHREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    MxOut mxo;
    mxo.q_hi = reinterpret_cast<unsigned char*>(o4_hi);
    mxo.q_lo = reinterpret_cast<unsigned char*>(o4_lo);
    mxo.s_hi = reinterpret_cast<unsigned char*>(so_hi);
    mxo.s_lo = reinterpret_cast<unsigned char*>(so_lo);
    if (gelu) gemm_et_x64p_kernel<PREC, false, true, false, false, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, 0, nullptr, nullptr, nullptr, nullptr, 0, mxo);
    else gemm_et_x64p_kernel<PREC, false, false, false, false, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, 0, nullptr, nullptr, nullptr, nullptr, 0, mxo);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// gemm_et_w4x_kernel (round 5): the vendor's tile geometry on this file's LDS-DMA pair stages -- 256 x 256 x 64 macro tile, FOUR waves
// with 512 registers each, wave tile 128 x 128 on v_mfma_f32_16x16x32 (the form tools/mfma_rate.hip measures 24 % faster than
// 32x32x16 in the bare pipe; the round-2 four-wave kernel above was built on 32x32x16).  VERDICT r04 item 1a.
//
//   * 64 accumulator tiles of 16 x 16 = 256 registers, ALL in AGPRs (inline-asm MFMAs with "+a"); the first k-step of a tile
//     writes them with C = 0, so no accumulator is ever zeroed by 256 v_accvgpr_write;
//   * per 32-k step and wave: 64 MFMAs (1024 pipe cycles), 16 ds_read_b128 (8 A + 8 B fragments: 0.25 per MFMA against 0.325 for the
//     128 x 80 wave tile of the eight-wave kernels), into the OTHER of two fragment register sets (128 VGPRs);
//   * a 64-k pair stage = 512 rows x 128 B = 64 KiB = 64 whole-line DMA pieces, 16 per wave, spread over the second step of the stage
//     one behind every second MFMA (a piece = s_mov m0 + the load; the per-piece source offset sits in eight VGPRs, the stage base
//     in two SGPR pairs);
//   * ONE block barrier per stage, between its two steps: before it every wave waits for its own pieces of stage t + 1 (issued a
//     whole stage earlier) and has finished reading stage t (its k-half 1 fragments were read during step 0); after it stage t + 2
//     goes into the buffer of stage t.  The stage stream runs on across tiles (persistent, one block per CU): the next tile's
//     stages 0 and 1 land under the last stage and the epilogue, which bounces through 17 KiB of LDS of its own.
// Same LDS image, swizzle and k order as gemm_et_x64_kernel: bit-identical output.  M % 256 == 0, N % 256 == 0, K % 64 == 0 (round 6: an
// odd number of stages per tile is fine -- the buffer parity simply carries over to the next tile).
// ---------------------------------------------------------------------------------------------
template <int PREC, bool ZERO>
__device__ __forceinline__ void mfma16_asm(f32x4_t& c, const uint4& a, const uint4& b) {
    const u32x4_t av = __builtin_bit_cast(u32x4_t, a), bv = __builtin_bit_cast(u32x4_t, b);
    if constexpr (PREC == PREC_F16) {
        if constexpr (ZERO) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, 0" : "=a"(c) : "v"(av), "v"(bv));
        else asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+a"(c) : "v"(av), "v"(bv));
    } else {
        if constexpr (ZERO) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=a"(c) : "v"(av), "v"(bv));
        else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(av), "v"(bv));
    }
}

constexpr int W4X_ROWS = QBM + W4X_BN;                 // 512 stage rows
constexpr int W4X_STAGE_ELEMS = W4X_ROWS * XBK;        // 64 KiB per stage
constexpr int W4X_SCR_BYTES = 4 * 16 * 272;            // epilogue scratch: per wave one m-tile of 16 rows x 272 B (epilogue_coalesced, NI = 8, JC = 1)

// ET outputs only: the fp32 epilogue bounces 8 KiB per wave and m-tile, which the 160 KiB do not hold next to two 64 KiB stages (and the
// fp32-output shapes of this path, N = 1280, are 2.5 rounds of 256 x 256 tiles: nothing to gain there).
template <int PREC, bool OUT_F32, int GELU, bool STREAM = false /* non-temporal output stores (stream_hidden) */>
__global__ __attribute__((amdgpu_flat_work_group_size(W4THREADS, W4THREADS), amdgpu_waves_per_eu(1, 1))) void gemm_et_w4x_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, void* __restrict__ Cv,
    const float* __restrict__ bias, int M, int N, int K, int accumulate, int ld = 0 /* row stride of A and B in elements, 0 = K */) {
    static_assert(!OUT_F32, "ET outputs only (epilogue scratch: 16 rows x 272 B per wave)");
    constexpr int NI = 8, NJ = 8;
    constexpr uint32_t XSB = W4X_STAGE_ELEMS * 2;
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * W4X_STAGE_ELEMS + W4X_SCR_BYTES / 2];   // 128 KiB ring + 17 KiB scratch, ONE object

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;               // wave tile rows wm*128.., cols wn*128..

    constexpr int GROUP = 8;
    const int tiles_n = N / W4X_BN, tiles_m = M / QBM, ntiles = tiles_n * tiles_m;
    const int per_group = GROUP * tiles_n;
#define W4X_TILE(L_, m_, n_)                                                                     \
    do {                                                                                         \
        const int bid_ = xcd_remap((L_), ntiles);                                                \
        const int group_ = bid_ / per_group, first_m_ = group_ * GROUP;                           \
        const int gsz_ = (tiles_m - first_m_) < GROUP ? (tiles_m - first_m_) : GROUP;            \
        const int in_g_ = bid_ - group_ * per_group;                                             \
        (m_) = (first_m_ + in_g_ % gsz_) * QBM;                                                  \
        (n_) = (in_g_ / gsz_) * W4X_BN;                                                          \
    } while (0)

    // DMA map: piece q of this wave covers stage rows 32 q + 8 wave .. + 7 (q < 8: A rows, else B rows 32 (q - 8) + ..); lane l ->
    // k-half l>>5, row (l>>2)&7, physical chunk l&3 (the image and swizzle of the eight-wave kernels: 32 q = 0 mod 16).  The byte
    // offset of (piece q & 7, lane) from the stage base is the same for A and B: eight VGPRs.
    const int LD = ld > 0 ? ld : K;                        // operand row stride (elements)
    const int prow = 8 * wave + ((lane >> 2) & 7);
    uint32_t voffq[8];
#pragma unroll
    for (int q = 0; q < 8; ++q)
        voffq[q] = ((uint32_t)(prow + 32 * q) * (uint32_t)LD + (uint32_t)(lane >> 5) * 32u + (uint32_t)qswz(prow, lane & 3) * 8u) * 2u;
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds + (uint32_t)wave * 1024u);
#define W4X_PIECE(pa_, pb_, wr_, q_) glds16_m(voffq[(q_) & 7], ((q_) < 8 ? (pa_) : (pb_)), lds0 + (wr_) + (q_) * 4096u)
#define W4X_ISSUE_ALL(pa_, pb_, wr_)                                                                       \
    do {                                                                                                   \
        W4X_PIECE(pa_, pb_, wr_, 0); W4X_PIECE(pa_, pb_, wr_, 1); W4X_PIECE(pa_, pb_, wr_, 2); W4X_PIECE(pa_, pb_, wr_, 3);     \
        W4X_PIECE(pa_, pb_, wr_, 4); W4X_PIECE(pa_, pb_, wr_, 5); W4X_PIECE(pa_, pb_, wr_, 6); W4X_PIECE(pa_, pb_, wr_, 7);     \
        W4X_PIECE(pa_, pb_, wr_, 8); W4X_PIECE(pa_, pb_, wr_, 9); W4X_PIECE(pa_, pb_, wr_, 10); W4X_PIECE(pa_, pb_, wr_, 11);   \
        W4X_PIECE(pa_, pb_, wr_, 12); W4X_PIECE(pa_, pb_, wr_, 13); W4X_PIECE(pa_, pb_, wr_, 14); W4X_PIECE(pa_, pb_, wr_, 15); \
    } while (0)

    const int nst = K / XBK;
    const int fr = lane & 15, fq = lane >> 4;
    // fragment BYTE offsets inside a stage for k-half 0; k-half 1 is +512
    uint32_t offA[NJ], offB[NI];
#pragma unroll
    for (int j = 0; j < NJ; ++j) { const int r = wm * 128 + j * 16 + fr; offA[j] = ((r >> 3) * 512 + (r & 7) * 32 + qswz(r, fq) * 8) * 2; }
#pragma unroll
    for (int i = 0; i < NI; ++i) { const int r = QBM + wn * 128 + i * 16 + fr; offB[i] = ((r >> 3) * 512 + (r & 7) * 32 + qswz(r, fq) * 8) * 2; }
    const unsigned char* ldsb = reinterpret_cast<const unsigned char*>(lds);
#define W4X_RDB(fb_, rd_, kh_, i_) fb_[i_] = *reinterpret_cast<const uint4*>(ldsb + (rd_) + (kh_) * 512 + offB[i_])
#define W4X_RDA(fa_, rd_, kh_, j_) fa_[j_] = *reinterpret_cast<const uint4*>(ldsb + (rd_) + (kh_) * 512 + offA[j_])
    // slot k (0 .. 63) of a 32-k step: MFMA on accumulator tile (i = k % 8, j = k / 8) of the set (ca_, cb_); slots 0 - 15: one read of
    // the NEXT step's set (na_, nb_) from buffer nrd_, k-half nkh_; D_ != 0: DMA piece (k - 16) / 2 behind the even slots 16 .. 46
    // when dma_ (wave-uniform) is set.  Z_: first step of a tile (C = 0).
#define W4X_SLOT(k_, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                          \
        mfma16_asm<PREC, Z_>(acc[(k_) % 8][(k_) / 8], cb_[(k_) % 8], ca_[(k_) / 8]);                       \
        if constexpr ((k_) < 8) { W4X_RDB(nb_, nrd_, nkh_, ((k_) < 8 ? (k_) : 0)); }                       \
        else if constexpr ((k_) < 16) { W4X_RDA(na_, nrd_, nkh_, ((k_) >= 8 && (k_) < 16 ? (k_) - 8 : 0)); } \
        if constexpr ((D_) != 0 && (k_) >= 16 && (k_) < 48 && ((k_) & 1) == 0) {                           \
            if (dma_) W4X_PIECE(pa_, pb_, wr_, ((k_) >= 16 && (k_) < 48 ? ((k_) - 16) / 2 : 0));           \
        }                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);
#define W4X_SLOT8(k_, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                         \
        W4X_SLOT((k_) + 0, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                    \
        W4X_SLOT((k_) + 1, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                    \
        W4X_SLOT((k_) + 2, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                    \
        W4X_SLOT((k_) + 3, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                    \
        W4X_SLOT((k_) + 4, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                    \
        W4X_SLOT((k_) + 5, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                    \
        W4X_SLOT((k_) + 6, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                    \
        W4X_SLOT((k_) + 7, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)
#define W4X_STEP(Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                              \
        W4X_SLOT8(0, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                          \
        W4X_SLOT8(8, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                          \
        W4X_SLOT8(16, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                         \
        W4X_SLOT8(24, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                         \
        W4X_SLOT8(32, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                         \
        W4X_SLOT8(40, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                         \
        W4X_SLOT8(48, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)                         \
        W4X_SLOT8(56, Z_, ca_, cb_, na_, nb_, nrd_, nkh_, D_, dma_, pa_, pb_, wr_)
    // one 64-k stage held in buffer rd; (da_, db_) = A / B rows of the stage that goes into this buffer two stages on (dma_: it exists)
#define W4X_STAGE(Z_, dma_, da_, db_)                                                                      \
        {                                                                                                  \
            const uint32_t ot = XSB - rd;                                                                  \
            W4X_STEP(Z_, fa0, fb0, fa1, fb1, rd, 1, 0, false, da_, db_, rd)                                \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                    \
            __builtin_amdgcn_s_barrier();                                                                  \
            __builtin_amdgcn_sched_barrier(0);                                                             \
            W4X_STEP(false, fa1, fb1, fa0, fb0, ot, 0, 1, dma_, da_, db_, rd)                              \
            rd = ot;                                                                                       \
        }

    int L = blockIdx.x, m0, n0;
    W4X_TILE(L, m0, n0);
    const uint16_t* sA = A + (size_t)m0 * LD;
    const uint16_t* sB = B + (size_t)n0 * LD;
    W4X_ISSUE_ALL(sA, sB, 0u);                             // stage 0 -> buffer 0
    {
        const uint16_t* a1 = sA + XBK;
        const uint16_t* b1 = sB + XBK;
        W4X_ISSUE_ALL(a1, b1, XSB);                        // stage 1 -> buffer 1 (lands under stage 0)
    }
    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");      // in-order retirement: the 16 pieces of stage 0 have landed
    __builtin_amdgcn_s_barrier();
    f32x4_t acc[NI][NJ];
    uint4 fa0[NJ], fb0[NI], fa1[NJ], fb1[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) W4X_RDB(fb0, 0u, 0, i);
#pragma unroll
    for (int j = 0; j < NJ; ++j) W4X_RDA(fa0, 0u, 0, j);
    __builtin_amdgcn_sched_barrier(0);
    uint32_t rd = 0;
    for (;;) {
        const int Ln = L + (int)gridDim.x;
        const bool more = Ln < ntiles;
        int m1 = m0, n1 = n0;
        if (more) W4X_TILE(Ln, m1, n1);
        const uint16_t* nA = A + (size_t)m1 * LD;
        const uint16_t* nB = B + (size_t)n1 * LD;
        // (rd lives across tiles: with an EVEN number of stages per tile it is back at 0 here -- the round-5 behaviour, bit for bit --, with
        // an odd number (K = 1344: the K = 1280 operands + the 64-column outlier extension, engine_encode.hip block_route) the next tile starts in buffer 1)
        // stage t feeds stage t + 2 into its own buffer; past the end of this tile that is stage t + 2 - nst of the NEXT tile
        const uint16_t* pa = sA + 2 * XBK;
        const uint16_t* pb = sB + 2 * XBK;
        W4X_STAGE(true, true, pa, pb)                      // t = 0 (nst >= 4: stage 2 exists)
        for (int t = 1; t + 2 < nst; ++t) {
            pa += XBK;
            pb += XBK;
            W4X_STAGE(false, true, pa, pb)
        }
        W4X_STAGE(false, more, nA, nB)                     // t = nst - 2 (buffer 0): the next tile's stage 0
        {
            const uint16_t* a1 = nA + XBK;
            const uint16_t* b1 = nB + XBK;
            W4X_STAGE(false, more, a1, b1)                 // t = nst - 1 (buffer 1): the next tile's stage 1; its step 1 reads that tile's stage 0
        }
        // The last MFMA results must not be read for 18 wait states, and hipcc does not know the asm statements above are MFMAs: the
        // padding is tied to every accumulator tile by data dependence (eight statements, one row of tiles each).
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (j == 0)
                asm volatile("s_nop 15\n\ts_nop 15" : "+a"(acc[0][j]), "+a"(acc[1][j]), "+a"(acc[2][j]), "+a"(acc[3][j]), "+a"(acc[4][j]),
                             "+a"(acc[5][j]), "+a"(acc[6][j]), "+a"(acc[7][j]));
            else
                asm volatile("" : "+a"(acc[0][j]), "+a"(acc[1][j]), "+a"(acc[2][j]), "+a"(acc[3][j]), "+a"(acc[4][j]), "+a"(acc[5][j]),
                             "+a"(acc[6][j]), "+a"(acc[7][j]));
        }
        __builtin_amdgcn_sched_barrier(0);
        {
            unsigned char* scr = reinterpret_cast<unsigned char*>(lds) + 2 * XSB + wave * (W4X_SCR_BYTES / 4);
            epilogue_coalesced<PREC, OUT_F32, GELU, NJ, 1, NI, false, false, STREAM>(acc, scr, Cv, bias, nullptr, 1, N, m0 + wm * 128, n0 + wn * 128, accumulate, lane);
        }
        if (!more) break;
        L = Ln; m0 = m1; n0 = n1; sA = nA; sB = nB;
    }
#undef W4X_TILE
#undef W4X_PIECE
#undef W4X_ISSUE_ALL
#undef W4X_RDA
#undef W4X_RDB
#undef W4X_SLOT
#undef W4X_SLOT8
#undef W4X_STEP
#undef W4X_STAGE
}

template <int PREC>
hipError_t launch_gemm_w4x(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, bool out_f32, bool gelu,
                           bool accumulate, int ld, int gelu_form, hipStream_t s) {
    const int ntiles = (M / QBM) * (N / W4X_BN);
    const int n_cu = cu_count();
    dim3 grid(ntiles > n_cu ? n_cu : ntiles), block(W4THREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    const int acc = accumulate ? 1 : 0;
    if (out_f32) return hipErrorInvalidValue;
    const bool so = gelu && stream_hidden(M, N);
    if (gelu && gelu_form == 2 && so) gemm_et_w4x_kernel<PREC, false, 2, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc, ld);
    else if (gelu && gelu_form == 2) gemm_et_w4x_kernel<PREC, false, 2><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc, ld);
    else if (gelu && so) gemm_et_w4x_kernel<PREC, false, 1, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc, ld);
    else if (gelu) gemm_et_w4x_kernel<PREC, false, 1><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc, ld);
    else gemm_et_w4x_kernel<PREC, false, 0><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc, ld);
    return hipGetLastError();
}

#ifdef SAMRS_EXPERIMENTS
// consumer: C (ET) = [GELU](rstd (Xh Wf^T - mean cvec) + bias_f) on the persistent pair-stage kernel
template <int PREC>
hipError_t launch_gemm_x64p_fold(const void* A, const void* B, void* C, const float* bias, const float* cvec, const float* rowstat,
                                 int M, int N, int K, bool gelu, hipStream_t s) {
    const int ntiles = (M / QBM) * (N / WBN);
    const int n_cu = cu_count_now();
    dim3 grid(ntiles < n_cu ? ntiles : n_cu), block(QTHREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    const float2* rs = reinterpret_cast<const float2*>(rowstat);
    if (gelu) gemm_et_x64p_kernel<PREC, false, true, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, 0, rs, cvec);
    else gemm_et_x64p_kernel<PREC, false, false, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, 0, rs, cvec);
    return hipGetLastError();
}
#endif  // SAMRS_EXPERIMENTS (fold launchers)
template <int PREC, int NI, int MODE>
hipError_t launch_gemm_x64(const void* A, const void* B, void* C, const float* bias, const float* add2d, int period,
                           int M, int N, int K, bool out_f32, bool gelu, bool accumulate, hipStream_t s) {
    dim3 grid((M / QBM) * (N / (64 * NI))), block(QTHREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    const int acc = accumulate ? 1 : 0;
    if (out_f32) {
        if (gelu) gemm_et_x64_kernel<PREC, true, true, NI, MODE><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc, g_x64_skew);
        else gemm_et_x64_kernel<PREC, true, false, NI, MODE><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc, g_x64_skew);
    } else {
        if (gelu) gemm_et_x64_kernel<PREC, false, true, NI, MODE><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc, g_x64_skew);
        else gemm_et_x64_kernel<PREC, false, false, NI, MODE><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc, g_x64_skew);
    }
    return hipGetLastError();
}

// proj / lin2 with the outlier-column stage (gemm_et_x64_kernel EXT): C (fp32) += A B^T + A_x B_x^T + bias
template <int PREC>
hipError_t launch_gemm_x64_ext(const void* A, const void* B, const void* Ax, const void* Bx, void* C, const float* bias,
                               int M, int N, int K, hipStream_t s) {
    dim3 grid((M / QBM) * (N / WBN)), block(QTHREADS);
    gemm_et_x64_kernel<PREC, true, false, 5, 3, 0, false, false, true><<<grid, block, 0, s>>>(
        reinterpret_cast<const uint16_t*>(A), reinterpret_cast<const uint16_t*>(B), C, bias, nullptr, 0, M, N, K, 1, g_x64_skew,
        reinterpret_cast<const uint16_t*>(Ax), reinterpret_cast<const uint16_t*>(Bx));
    return hipGetLastError();
}

template <int PREC, int NI = 4>
hipError_t launch_gemm_big(const void* A, const void* B, void* C, const float* bias, const float* add2d, int period,
                           int M, int N, int K, bool out_f32, bool gelu, bool accumulate, hipStream_t s) {
    dim3 grid((M / QBM) * (N / (64 * NI))), block(QTHREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    const int acc = accumulate ? 1 : 0;
    if (out_f32) {
        if (gelu) gemm_et_big_kernel<PREC, true, true, 0, NI><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
        else gemm_et_big_kernel<PREC, true, false, 0, NI><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
    } else {
        if (gelu) gemm_et_big_kernel<PREC, false, true, 0, NI><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
        else gemm_et_big_kernel<PREC, false, false, 0, NI><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, acc);
    }
    return hipGetLastError();
}


thread_local int tl_gemm_variant = -1;   // per-engine override, set around an engine's launches (engine_state.h GemmVariantScope)
int g_gemm_variant = 8;   // 0 reg-staged 128^2, 1 +LDS-DMA, 2 +grouped order, 3 reg+grouped, 4 256x128 3-stage pipe, 5 +staggered groups, 6 256x256, 7 2 blocks/CU, 8 auto(5|6|7)


// =============================================================================================================================
// MXFP4 lo terms (round 4).  The operand split  A B^T ~= A_hi B_hi^T + A_lo B_hi^T + A_hi B_lo^T  pays two extra f16 passes for
// corrections that are 2^-11 of the product.  Their operands tolerate very few mantissa bits (oracle/error_budget.py plans8 - 10:
// e2m1 lo terms leave 1.8e-1 of a plain f16 GEMM's error, and the C4 floor of the multimask mode holds with them), so here the
// two correction terms run on gfx950's block-scaled  v_mfma_scale_f32_16x16x128_f8f6f4  with FP4 (e2m1) operands and one E8M0
// scale per 32 k (OCP MX): 4x the f16 MFMA rate -- and, the reason for fp4 rather than fp8 / fp6, the SAME LDS geometry as the
// f16 stage: a 128-byte stage row holds 256 k of fp4 (two 64-byte k-halves of 128 k each) where it holds 64 k of f16, and a
// lane's fragment of a k-half is the same 16 bytes (32 fp4 values = its MX block) it is for f16.  So the pair-stage image, its
// XOR swizzle, the DMA map, the 13 fragment reads and the 40 MFMAs per k-half are those of gemm_et_x64_kernel; an MX stage
// differs in the MFMA opcode, in two 8-byte scale reads per k-half, and in six 1-KiB scale pieces per stage.  A correction
// segment over K is K / 256 stages against K / 64 for the f16 segment: the split product costs 1.5x a plain one (f16 lo: 3x).
//
// Operand tensors (written by mx4_pack_kernel, or by the producers themselves):
//   A4 / B4  [rows][Kp / 2] bytes: element k' of a row in nibble k' (low nibble first); Kp = padded K (a multiple of 256)
//   scales   E8M0 bytes, one per (row, 32-k' block), stored in the order the kernel's lanes read them:
//              A: [tile_m = r / 256][stage = b / 8][k-half = (b / 4) % 2][wm = (r / 128) % 2][fq = b % 4][fr = r % 16][j = (r / 16) % 8]
//              B: [tile_n = n / 320][stage][k-half][wn = (n / 80) % 4][fq][fr = n % 16][i = (n % 80) / 16, 8 slots]
//            i.e. 2 KiB / 4 KiB per (tile, stage), DMA'd as they are; lane (fr, fq) of wave (wm, wn) reads 8 bytes per operand and
//            k-half, byte j / i = the scale of its row in m-tile j / n-tile i (op_sel picks the byte).
// K' may be K with each group of G elements padded to GP (heads of 80 padded to 96 for the proj GEMM: no MX block straddles two
// heads, so the attention kernels can emit the blocks of their own head); the f16 segment keeps the plain K.
// =============================================================================================================================
constexpr int MX_S_BYTES = MX_SA_BYTES + MX_SB_BYTES;          // MXK, MX_SA_BYTES, MX_SB_BYTES and the quantisers: common.h

struct MxOperands {
    const unsigned char *a4_lo, *a4_hi, *b4_hi, *b4_lo;      // fp4 data
    const unsigned char *sa_lo, *sa_hi, *sb_hi, *sb_lo;      // scale tiles
    int Kp;                                                  // padded K of the MX segments
    int split_from_n;                                        // output columns below this take no lo terms (ET outputs; 0 = all do)
};

typedef int mx_v8i __attribute__((ext_vector_type(8)));
typedef int mx_v4i __attribute__((ext_vector_type(4)));

template <int OPA, int OPB>
__device__ __forceinline__ f32x4_t mfma_mx4(const uint4& a, const uint4& b, f32x4_t c, int sa, int sb) {
    const mx_v4i xa = {(int)a.x, (int)a.y, (int)a.z, (int)a.w}, xb = {(int)b.x, (int)b.y, (int)b.z, (int)b.w};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(__builtin_shufflevector(xa, xa, 0, 1, 2, 3, -1, -1, -1, -1),
                                                            __builtin_shufflevector(xb, xb, 0, 1, 2, 3, -1, -1, -1, -1), c,
                                                            4 /* fp4 e2m1 */, 4, OPA, sa, OPB, sb);
}

template <int PREC, bool OUT_F32, bool GELU = false, bool MXO = false>
__global__ __launch_bounds__(QTHREADS) void gemm_et_mx_kernel(
    const uint16_t* __restrict__ A, const uint16_t* __restrict__ B, void* __restrict__ Cv, const float* __restrict__ bias,
    int M, int N, int K, int accumulate, MxOperands mx, MxOut mxo = MxOut(),
    int ld = 0 /* row stride of A and B in elements, 0 = K */,
    int ext = 0 /* round 6: the rows carry the 64-column outlier extension behind their K live columns (engine_state.h EncBlock::oc_*): the tiles
                   that take NO lo terms (n0 < split_from_n: q and k of the v-third split) read it as one more f16 stage; the tiles that do
                   take them are covered by their fp4 correction segments, which span every column */) {
    constexpr int NI = 5;
    constexpr int XBN = 64 * NI;
    constexpr int XROWS = QBM + XBN;
    constexpr int XSTAGE_ELEMS = XROWS * XBK;
    constexpr uint32_t XSB = XSTAGE_ELEMS * 2;             // stage bytes (f16 and MX alike: rows x 128 B)
    __shared__ __attribute__((aligned(16))) uint16_t lds[2 * XSTAGE_ELEMS + MX_S_BYTES];   // ring (144 KiB) + 2 x 6 KiB of scales
    const int LD = ld > 0 ? ld : K;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave >> 2;
    const int wm = wave >> 2, wn = wave & 3;

    // PERSISTENT as gemm_et_x64p_kernel: a block walks tiles L, L + gridDim.x, ...; the next tile's stage 0 (and its scale tiles) goes
    // out before the epilogue, whose bounce scratch is confined to ring buffer 1.  (A grid of one block per tile degenerates to
    // the one-tile kernel: SAMRS_MX_PERSIST=0, kept for A/B runs.)
    constexpr int GROUP = 8;
    const int tiles_n = N / XBN, tiles_m = M / QBM, ntiles = tiles_n * tiles_m;
    const int per_group = GROUP * tiles_n;
#define MX_TILE(L_, tm_, tn_)                                                                    \
    do {                                                                                         \
        const int bid_ = xcd_remap((L_), ntiles);                                                \
        const int group_ = bid_ / per_group, first_m_ = group_ * GROUP;                           \
        const int gsz_ = (tiles_m - first_m_) < GROUP ? (tiles_m - first_m_) : GROUP;            \
        const int in_g_ = bid_ - group_ * per_group;                                             \
        (tm_) = first_m_ + in_g_ % gsz_;                                                         \
        (tn_) = in_g_ / gsz_;                                                                    \
    } while (0)
    int L = blockIdx.x, tile_m, tile_n;                    // the tile being FED (the DMA macros below read these)
    MX_TILE(L, tile_m, tile_n);
    int m0 = tile_m * QBM, n0 = tile_n * XBN;              // the tile being COMPUTED (epilogue)

    const int nst1 = K / XBK;                              // f16 stages
    const int nst4 = mx.Kp / MXK;                          // MX stages per correction segment
    int nmx = n0 >= mx.split_from_n ? 2 * nst4 : 0;        // MX stages of the tile being fed (wave-uniform): A_lo B_hi, then A_hi B_lo
    int nf16 = nst1 + ((ext && n0 < mx.split_from_n) ? 1 : 0);   // ... and its f16 stages (+ the outlier extension where no lo terms run)

    // DMA map as in gemm_et_x64_kernel; the per-lane byte offset depends on the row stride of the source (2 K vs Kp / 2)
    const int prow = 8 * wave + ((lane >> 2) & 7);
    const uint32_t lane_off = (uint32_t)(lane >> 5) * 64u + (uint32_t)qswz(prow, lane & 3) * 16u;
    const uint32_t voff16 = (uint32_t)prow * (uint32_t)LD * 2u + lane_off;
    const uint32_t voff4 = (uint32_t)prow * (uint32_t)(mx.Kp >> 1) + lane_off;
    const unsigned char* A16 = reinterpret_cast<const unsigned char*>(A) + (size_t)m0 * LD * 2;     // of the tile being fed
    const unsigned char* B16 = reinterpret_cast<const unsigned char*>(B) + (size_t)n0 * LD * 2;
    int fm0 = m0, fn0 = n0;                                // rows of the tile being fed (the fp4 sources)
    const size_t row4 = (size_t)(mx.Kp >> 1);
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds + (uint32_t)wave * 1024u);
    const uint32_t lds_sc = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(__attribute__((address_space(3))) void*)lds + 2u * XSB);
    // piece q_ (literal) of stage st_ into the ring buffer at byte offset wr_ (scales: buffer (wr_ != 0))
#define MX_PIECE(st_, wr_, q_)                                                                                       \
    do {                                                                                                             \
        const int st__ = (st_);                                                                                      \
        /* readfirstlane: inside the persistent loop LLVM moves some wave-uniform address chains to VGPRs (SGPR pressure) and */ \
        /* then hands the VGPR to the "s" operand of the inline asm ("s_mov_b32 m0, v0": does not assemble)                   */ \
        const uint32_t dst__ = __builtin_amdgcn_readfirstlane(                                                       \
            lds0 + (wr_) + ((q_) < 4 ? (q_) * 8192u : (uint32_t)(QBM * XBK * 2) + ((q_) - 4) * 8192u));              \
        if (st__ < nmx) {                                                                                            \
            const int seg__ = st__ >= nst4, s__ = st__ - seg__ * nst4;                                               \
            const unsigned char* src__ = (q_) < 4 ? (seg__ ? mx.a4_hi : mx.a4_lo) + ((size_t)fm0 + (q_) * 64) * row4         \
                                                   : (seg__ ? mx.b4_lo : mx.b4_hi) + ((size_t)fn0 + ((q_) - 4) * 64) * row4; \
            glds16_s(voff4, src__ + (size_t)s__ * 128, dst__);                                                       \
        } else {                                                                                                     \
            const unsigned char* src__ = (q_) < 4 ? A16 + (size_t)(q_) * 64 * LD * 2 : B16 + (size_t)((q_) - 4) * 64 * LD * 2; \
            glds16_s(voff16, src__ + (size_t)(st__ - nmx) * 128, dst__);                                             \
        }                                                                                                            \
    } while (0)
    // the stage's scale tiles: 2 KiB (A) + 4 KiB (B) as six 1-KiB pieces, one per wave 0 .. 5
#define MX_SCALES(st_, wr_)                                                                                          \
    do {                                                                                                             \
        const int st__ = (st_);                                                                                      \
        if (st__ < nmx && wave < 6) {                                                                                \
            const int seg__ = st__ >= nst4, s__ = st__ - seg__ * nst4;                                               \
            const unsigned char* src__ = wave < 2                                                                    \
                ? (seg__ ? mx.sa_hi : mx.sa_lo) + ((size_t)tile_m * nst4 + s__) * MX_SA_BYTES + wave * 1024          \
                : (seg__ ? mx.sb_lo : mx.sb_hi) + ((size_t)tile_n * nst4 + s__) * MX_SB_BYTES + (wave - 2) * 1024;   \
            glds16_s((uint32_t)lane * 16u, src__,                                                                    \
                     __builtin_amdgcn_readfirstlane(lds_sc + ((wr_) ? (uint32_t)MX_S_BYTES : 0u) + (uint32_t)wave * 1024u)); \
        }                                                                                                            \
    } while (0)
#define MX_ISSUE(st_, wr_)                                                                                           \
    do {                                                                                                             \
        MX_PIECE(st_, wr_, 0); MX_PIECE(st_, wr_, 1); MX_PIECE(st_, wr_, 2); MX_PIECE(st_, wr_, 3); MX_PIECE(st_, wr_, 4); \
        MX_PIECE(st_, wr_, 5); MX_PIECE(st_, wr_, 6); MX_PIECE(st_, wr_, 7); MX_PIECE(st_, wr_, 8); MX_SCALES(st_, wr_); \
    } while (0)

    f32x4_t acc[NI][8];

    const int fr = lane & 15, fq = lane >> 4;
    uint32_t offA[8], offB[NI];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const int r = wm * 128 + j * 16 + fr; offA[j] = ((r >> 3) * 512 + (r & 7) * 32 + qswz(r, fq) * 8) * 2; }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int r = QBM + wn * (16 * NI) + i * 16 + fr;
        offB[i] = ((r >> 3) * 512 + (r & 7) * 32 + qswz(r, fq) * 8) * 2;
    }
    const unsigned char* ldsb = reinterpret_cast<const unsigned char*>(lds);
    const uint32_t scA = 2u * XSB + (uint32_t)((wm * 64 + fq * 16 + fr) * 8);                    // + kh * 1024 + buffer * MX_S_BYTES
    const uint32_t scB = 2u * XSB + (uint32_t)MX_SA_BYTES + (uint32_t)((wn * 64 + fq * 16 + fr) * 8);   // + kh * 2048 + ...

    MX_ISSUE(0, 0u);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

#define MX_READ(rd_, kh_)                                                                                  \
    _Pragma("unroll") for (int i = 0; i < NI; ++i)                                                         \
        fb[i] = *reinterpret_cast<const uint4*>(ldsb + (rd_) + (kh_) * 512 + offB[i]);                     \
    _Pragma("unroll") for (int j = 0; j < 8; ++j)                                                          \
        fa[j] = *reinterpret_cast<const uint4*>(ldsb + (rd_) + (kh_) * 512 + offA[j]);
#define MX_READ_SC(rd_, kh_)                                                                               \
    sa = *reinterpret_cast<const uint2*>(ldsb + scA + ((rd_) ? (uint32_t)MX_S_BYTES : 0u) + (kh_) * 1024); \
    sb = *reinterpret_cast<const uint2*>(ldsb + scB + ((rd_) ? (uint32_t)MX_S_BYTES : 0u) + (kh_) * 2048);
    // one row of MFMAs (m-tile j_) + the DMA piece that rides behind it
#define MX_DMA_AFTER(j_, dma_, st_, wr_)                                                                   \
    if (dma_) {                                                                                            \
        if ((j_) == 0) MX_PIECE(st_, wr_, 0); if ((j_) == 1) MX_PIECE(st_, wr_, 1);                        \
        if ((j_) == 2) MX_PIECE(st_, wr_, 2); if ((j_) == 3) MX_PIECE(st_, wr_, 3);                        \
        if ((j_) == 4) MX_PIECE(st_, wr_, 4); if ((j_) == 5) MX_PIECE(st_, wr_, 5);                        \
        if ((j_) == 6) { MX_PIECE(st_, wr_, 6); MX_SCALES(st_, wr_); }                                     \
        if ((j_) == 7) { MX_PIECE(st_, wr_, 7); MX_PIECE(st_, wr_, 8); }                                   \
    }
#define MX_MFMA_F16(dma_, st_, wr_)                                                                        \
    _Pragma("unroll") for (int j = 0; j < 8; ++j) {                                                        \
        _Pragma("unroll") for (int i = 0; i < NI; ++i) acc[i][j] = ET<PREC>::mfma16(fb[i], fa[j], acc[i][j]); \
        MX_DMA_AFTER(j, dma_, st_, wr_)                                                                    \
    }
    // first MFMA operand = the weight fragment (n rows): its scale is the B scale, byte i; second = activation fragment, byte j
#define MX_ROW(j_, OPB_, sav_)                                                                             \
    acc[0][j_] = mfma_mx4<0, OPB_>(fb[0], fa[j_], acc[0][j_], (int)sb.x, (int)(sav_));                     \
    acc[1][j_] = mfma_mx4<1, OPB_>(fb[1], fa[j_], acc[1][j_], (int)sb.x, (int)(sav_));                     \
    acc[2][j_] = mfma_mx4<2, OPB_>(fb[2], fa[j_], acc[2][j_], (int)sb.x, (int)(sav_));                     \
    acc[3][j_] = mfma_mx4<3, OPB_>(fb[3], fa[j_], acc[3][j_], (int)sb.x, (int)(sav_));                     \
    acc[4][j_] = mfma_mx4<0, OPB_>(fb[4], fa[j_], acc[4][j_], (int)sb.y, (int)(sav_));                     \
    /* pin the row here: unlike the plain MFMA intrinsics the scaled one is not convergent, and LLVM sinks all 80 of a stage */ \
    /* below the (branchy) DMA pieces that are meant to ride between the rows -- two k-halves of fragments live, 670 spills */  \
    asm volatile("" : "+v"(acc[0][j_]), "+v"(acc[1][j_]), "+v"(acc[2][j_]), "+v"(acc[3][j_]), "+v"(acc[4][j_]));
#define MX_MFMA_FP4(dma_, st_, wr_)                                                                        \
    MX_ROW(0, 0, sa.x) MX_DMA_AFTER(0, dma_, st_, wr_) MX_ROW(1, 1, sa.x) MX_DMA_AFTER(1, dma_, st_, wr_)  \
    MX_ROW(2, 2, sa.x) MX_DMA_AFTER(2, dma_, st_, wr_) MX_ROW(3, 3, sa.x) MX_DMA_AFTER(3, dma_, st_, wr_)  \
    MX_ROW(4, 0, sa.y) MX_DMA_AFTER(4, dma_, st_, wr_) MX_ROW(5, 1, sa.y) MX_DMA_AFTER(5, dma_, st_, wr_)  \
    MX_ROW(6, 2, sa.y) MX_DMA_AFTER(6, dma_, st_, wr_) MX_ROW(7, 3, sa.y) MX_DMA_AFTER(7, dma_, st_, wr_)

    // One stage (the schedule of gemm_et_x64_kernel<MODE = 3>: one block barrier per stage, DMA pieces spread between the MFMA
    // rows, the two wave groups half a stage apart).  The MX stages and the f16 stages run in two consecutive loops -- one MFMA
    // flavour per loop body; a single loop with a per-stage branch made the register allocator spill 670 registers -- and the
    // hand-over between them needs nothing: MX_PIECE decides per TARGET stage what it fetches.
#define MX_STAGE(READ_SC0_, READ_SC1_, MFMA_)                                                              \
    {                                                                                                      \
        uint4 fa[8], fb[NI];                                                                               \
        const uint32_t wr = XSB - rd;                                                                      \
        const bool dma0 = (grp == 0) && (t + 1 < nst);                                                     \
        const bool dma1 = (grp == 1) && (t + 2 < nst);                                                     \
        if (grp == 0) __builtin_amdgcn_s_barrier();                           /* R_t */                    \
        MX_READ(rd, 0)                                                                                     \
        READ_SC0_                                                                                          \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        __builtin_amdgcn_s_setprio(1);                                                                     \
        MFMA_(dma0, t + 1, wr)                                                                             \
        __builtin_amdgcn_s_setprio(0);                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        MX_READ(rd, 1)                                                                                     \
        READ_SC1_                                                                                          \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                 \
        if (grp == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        if (grp == 1) __builtin_amdgcn_s_barrier();       /* R_{t+1} of group 1: buffer rd is free from here on */ \
        __builtin_amdgcn_s_setprio(1);                                                                     \
        MFMA_(dma1, t + 2, rd)                                                                             \
        __builtin_amdgcn_s_setprio(0);                                                                     \
        if (grp == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        rd = wr;                                                                                           \
    }
    for (;;) {
        const int nst = nmx + nf16;                        // stages of THIS tile (the feed variables still are its own here)
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        if (grp == 1) {                                    // rendezvous R_0 of group 1; its share of stage 1 goes out first
            if (nst > 1) MX_ISSUE(1, XSB);
            __builtin_amdgcn_s_barrier();
        }
        uint32_t rd = 0;
        int t = 0;
        for (; t < nmx; ++t) {
            uint2 sa, sb;
            MX_STAGE(MX_READ_SC(rd, 0), MX_READ_SC(rd, 1), MX_MFMA_FP4)
        }
        for (; t < nst; ++t) MX_STAGE(, , MX_MFMA_F16)
        if (grp == 0) __builtin_amdgcn_s_barrier();        // both groups: same barrier count; every ring read of this tile is done

        // next tile: its stage 0 (fp4 or f16 pieces + the scale tiles) goes into ring buffer 0 / scale buffer 0 now and lands
        // under the epilogue
        const int Ln = L + (int)gridDim.x;
        const bool more = Ln < ntiles;
        const int em0 = m0, en0 = n0;
        if (more) {
            MX_TILE(Ln, tile_m, tile_n);
            fm0 = tile_m * QBM; fn0 = tile_n * XBN;
            A16 = reinterpret_cast<const unsigned char*>(A) + (size_t)fm0 * LD * 2;
            B16 = reinterpret_cast<const unsigned char*>(B) + (size_t)fn0 * LD * 2;
            nmx = fn0 >= mx.split_from_n ? 2 * nst4 : 0;
            nf16 = nst1 + ((ext && fn0 < mx.split_from_n) ? 1 : 0);
            MX_ISSUE(0, 0u);
        }
        {   // epilogue of tile (em0, en0); bounce scratch = ring buffer 1 only (72 KiB: 9 KiB per wave / 18 KiB per pair)
            unsigned char* upper = reinterpret_cast<unsigned char*>(lds) + XSB;
            if constexpr (!OUT_F32) {
                epilogue_pair_et<PREC, GELU, 2, true, false, MXO>(acc, upper, Cv, bias, nullptr, 1, N, em0 + wm * 128, en0 + (wn >> 1) * 160,
                                                                  wm, wn, lane, nullptr, nullptr, mxo);
            } else {
                epilogue_coalesced<PREC, true, false, 8, 1, NI, false, true>(acc, upper + wave * (XSB / 8), Cv, bias, nullptr, 1, N,
                                                                            em0 + wm * 128, en0 + wn * (16 * NI), accumulate, lane);
            }
        }
        if (!more) break;
        __builtin_amdgcn_s_barrier();          // scratch free again; stage 0 visible (each wave drained its pieces before its first store)
        L = Ln; m0 = fm0; n0 = fn0;
    }
#undef MX_STAGE
#undef MX_TILE
#undef MX_PIECE
#undef MX_SCALES
#undef MX_ISSUE
#undef MX_READ
#undef MX_READ_SC
#undef MX_DMA_AFTER
#undef MX_MFMA_F16
#undef MX_ROW
#undef MX_MFMA_FP4
}

// One (row, 32-k' block) per 8 lanes, 4 elements per lane.  Source: fp32 x (SRC_F32: hi = ET(x), lo = x - hi; also writes the ET
// copy when out_hi is given) or the ET pair (hi, lo) an existing producer wrote.  k' = padded index: group g = k' / GP holds the
// G source elements g G .. g G + G - 1 followed by GP - G zeros.
template <int PREC, bool SRC_F32>
__global__ __launch_bounds__(256) void mx4_pack_kernel(const float* __restrict__ x, const uint16_t* __restrict__ hi_in,
                                                       const uint16_t* __restrict__ lo_in, uint16_t* __restrict__ out_hi,
                                                       unsigned char* __restrict__ q_hi, unsigned char* __restrict__ q_lo,
                                                       unsigned char* __restrict__ s_hi, unsigned char* __restrict__ s_lo,
                                                       int rows, int K, int G, int GP, int is_b, int perm) {
    const int Kp = (K / G) * GP, nblk = Kp / 32, nst4 = Kp / MXK;
    const long item = ((long)blockIdx.x * 256 + threadIdx.x) >> 3;           // (row, block)
    const int sub = threadIdx.x & 7;
    if (item >= (long)rows * nblk) return;
    const int r = (int)(item / nblk), b = (int)(item % nblk);
    // position 4 sub .. 4 sub + 3 of the block holds source elements at block offset 4 sub (natural order) or 8 (sub & 3) + 4 (sub >> 2)
    // (perm: the order store_attention_row_mx writes its rows in)
    // perm 2: the order of epilogue_pair_et<MXO> (position 8 fq + 4 ib + e holds column 16 ib + 4 fq + e; sub = 2 fq + ib)
    const int in_blk = perm == 1 ? 8 * (sub & 3) + 4 * (sub >> 2) : perm == 2 ? 16 * (sub & 1) + 4 * (sub >> 1) : sub * 4;
    const int kp = b * 32 + in_blk, g = kp / GP, off = kp % GP;             // GP % 4 == 0 and G % 4 == 0: a lane's 4 elements share a fate
    float h[4] = {0.f, 0.f, 0.f, 0.f}, l[4] = {0.f, 0.f, 0.f, 0.f};
    if (off < G) {
        const size_t src = (size_t)r * K + (size_t)g * G + off;
        if constexpr (SRC_F32) {
            const float4 v = *reinterpret_cast<const float4*>(x + src);
            const float vv[4] = {v.x, v.y, v.z, v.w};
            uint2 hb;
            hb.x = pack2<PREC>(vv[0], vv[1]); hb.y = pack2<PREC>(vv[2], vv[3]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                h[e] = ET<PREC>::to_float((uint16_t)(((e & 2) ? hb.y : hb.x) >> (16 * (e & 1))));
                l[e] = vv[e] - h[e];
            }
            if (out_hi) *reinterpret_cast<uint2*>(out_hi + src) = hb;
        } else {
            const uint2 hb = *reinterpret_cast<const uint2*>(hi_in + src), lb = *reinterpret_cast<const uint2*>(lo_in + src);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                h[e] = ET<PREC>::to_float((uint16_t)(((e & 2) ? hb.y : hb.x) >> (16 * (e & 1))));
                l[e] = ET<PREC>::to_float((uint16_t)(((e & 2) ? lb.y : lb.x) >> (16 * (e & 1))));
            }
        }
    }
    float ah = fmaxf(fmaxf(fabsf(h[0]), fabsf(h[1])), fmaxf(fabsf(h[2]), fabsf(h[3])));
    float al = fmaxf(fmaxf(fabsf(l[0]), fabsf(l[1])), fmaxf(fabsf(l[2]), fabsf(l[3])));
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) { ah = fmaxf(ah, __shfl_xor(ah, o, 64)); al = fmaxf(al, __shfl_xor(al, o, 64)); }
    const int bh = mx_scale_byte(ah), bl = mx_scale_byte(al);
    const uint32_t ch = fp4_pack4(h[0], h[1], h[2], h[3], bh), cl = fp4_pack4(l[0], l[1], l[2], l[3], bl);
    const size_t dst = (size_t)r * (Kp / 2) + (size_t)b * 16 + sub * 2;
    *reinterpret_cast<uint16_t*>(q_hi + dst) = (uint16_t)ch;
    *reinterpret_cast<uint16_t*>(q_lo + dst) = (uint16_t)cl;
    if (sub == 0) {
        const size_t si = mx_scale_index(is_b != 0, r, b, nst4);
        s_hi[si] = (unsigned char)bh;
        s_lo[si] = (unsigned char)bl;
    }
}

}  // namespace

// what the selection rule (gemm_select.h) reads from the process
static GemmEnv gemm_env() {
    static const bool once = [] {          // tuning knob for A/B runs: SAMRS_GEMM_VARIANT=<n>
        if (const char* v = getenv("SAMRS_GEMM_VARIANT")) g_gemm_variant = atoi(v);
        return true;
    }();
    (void)once;
    static const bool w4x_auto = [] { const char* v = getenv("SAMRS_GEMM_W4X"); return v ? atoi(v) != 0 : true; }();
    GemmEnv e;
    // an engine handle's own choice (samrs_set_option "gemm_variant") overrides the process-wide test hook for its launches
    e.variant = tl_gemm_variant >= 0 ? tl_gemm_variant : g_gemm_variant;
    e.w4x_auto = w4x_auto;
#ifdef SAMRS_EXPERIMENTS
    static const int m32_mask = [] { const char* v = getenv("SAMRS_GEMM_M32"); return v ? atoi(v) : 0; }();
    e.m32_mask = m32_mask;
    e.experiments = true;
#else
    e.m32_mask = 0;
    e.experiments = false;       // the 32x32x16 kernels and the ablations are not in this build (make EXPERIMENTS=1)
#endif
    return e;
}
bool gemm_ld_ok(int M, int N, int K, bool gelu) { return gemm_plan_ld_ok(M, N, K, gelu, gemm_env()); }
bool gemm_ext_ok(int M, int N, int K) { return gemm_plan_ext_ok(M, N, K, gemm_env()); }
bool gemm_lntail_ok(int M, int N, int K) { return gemm_plan_lntail_ok(M, N, K, gemm_env()); }

// the rule's answer for a call, without a launch (samrs_debug_gemm_choice): out8 = kernel, ni, mode, persistent, reject, and what the
// three planning predicates say of the shape under the same variant
void gemm_debug_choice(int prec, int M, int N, int K, bool out_f32, bool gelu, bool accumulate, bool has_add2d, int ld, int variant,
                       int32_t* out8) {
    GemmEnv e = gemm_env();
    e.variant = variant;
    const GemmChoice ch = gemm_select(GemmCall{M, N, K, out_f32, gelu, accumulate, has_add2d, ld, prec == PREC_F16}, e);
    out8[0] = (int32_t)ch.kernel; out8[1] = ch.ni; out8[2] = ch.mode; out8[3] = ch.persistent ? 1 : 0;
    out8[4] = (ch.reject || (prec != PREC_F16 && prec != PREC_BF16)) ? 1 : 0;
    out8[5] = gemm_plan_ld_ok(M, N, K, gelu, e) ? 1 : 0; out8[6] = gemm_plan_ext_ok(M, N, K, e) ? 1 : 0; out8[7] = gemm_plan_lntail_ok(M, N, K, e) ? 1 : 0;
}

hipError_t launch_gemm_et_ext(int prec, const void* A, const void* B, const void* Ax, const void* Bx, float* C, const float* bias,
                              int M, int N, int K, hipStream_t s) {
    if (!A || !B || !Ax || !Bx || !C || !gemm_ext_ok(M, N, K)) return hipErrorInvalidValue;
    return with_prec(prec, [&](auto P) { return launch_gemm_x64_ext<P.value>(A, B, Ax, Bx, C, bias, M, N, K, s); });
}

#ifdef SAMRS_EXPERIMENTS
// the timing ablations (f16, ET output, no GELU): one instantiation per ablation number
static hipError_t launch_gemm_abl(const GemmChoice& ch, const void* A, const void* B, void* C, const float* bias, const float* add2d,
                                  int period, int M, int N, int K, hipStream_t s) {
    const bool big = ch.kernel == GemmKernel::ABL_BIG;
    dim3 grid((M / QBM) * (N / (big ? QBN : WBN))), block(QTHREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
#define ABL_CASE(x) case x: gemm_et_big_kernel<PREC_F16, false, false, x><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, 0); break;
#define XABL_CASE(x) case x: gemm_et_x64_kernel<PREC_F16, false, false, 5, 3, x><<<grid, block, 0, s>>>(a, b, C, bias, add2d, period, M, N, K, 0, g_x64_skew); break;
    if (big) switch (ch.abl) {
        ABL_CASE(0) ABL_CASE(1) ABL_CASE(4) ABL_CASE(6) ABL_CASE(8) ABL_CASE(7) ABL_CASE(16) ABL_CASE(22) ABL_CASE(23) ABL_CASE(24)
        default: return hipErrorInvalidValue;
    } else switch (ch.abl) {
        XABL_CASE(0) XABL_CASE(1) XABL_CASE(2) XABL_CASE(4) XABL_CASE(16) XABL_CASE(6) XABL_CASE(7) XABL_CASE(22) XABL_CASE(23) XABL_CASE(17)
        XABL_CASE(32) XABL_CASE(33) XABL_CASE(64)
        default: return hipErrorInvalidValue;
    }
#undef ABL_CASE
#undef XABL_CASE
    return hipGetLastError();
}
#endif

hipError_t launch_gemm_et(int prec, const void* A, const void* B, void* C, const float* bias,
                          const float* add2d, int add2d_period, int M, int N, int K, bool out_f32,
                          bool gelu, bool accumulate, hipStream_t s, GemmOpts opts) {
    if (add2d && add2d_period <= 0) return hipErrorInvalidValue;
    const GemmChoice ch = gemm_select(GemmCall{M, N, K, out_f32, gelu, accumulate, add2d != nullptr, opts.ld, prec == PREC_F16}, gemm_env());
    if (ch.reject) return hipErrorInvalidValue;
    return with_prec(prec, [&](auto P) -> hipError_t {
        constexpr int PR = P.value;
        auto x64 = [&](auto NI, auto MODE) {
            return launch_gemm_x64<PR, NI.value, MODE.value>(A, B, C, bias, add2d, add2d_period, M, N, K, out_f32, gelu, accumulate, s);
        };
        switch (ch.kernel) {
            case GemmKernel::BASE: return gemm_fam::base(prec, ch.glds, ch.group_m, A, B, C, bias, add2d, add2d_period, M, N, K, out_f32, gelu, accumulate, s);
            case GemmKernel::STAG: return gemm_fam::stag(prec, A, B, C, bias, add2d, add2d_period, M, N, K, out_f32, gelu, accumulate, s);
            case GemmKernel::DUAL: return gemm_fam::dual(prec, true, A, B, C, bias, add2d, add2d_period, M, N, K, out_f32, gelu, accumulate, s);
            case GemmKernel::DUAL_LOCKSTEP: return gemm_fam::dual(prec, false, A, B, C, bias, add2d, add2d_period, M, N, K, out_f32, gelu, accumulate, s);
            case GemmKernel::STAG_256x256: return launch_gemm_big<PR>(A, B, C, bias, add2d, add2d_period, M, N, K, out_f32, gelu, accumulate, s);
            case GemmKernel::STAG_256x320: return launch_gemm_big<PR, 5>(A, B, C, bias, add2d, add2d_period, M, N, K, out_f32, gelu, accumulate, s);
            case GemmKernel::X64:
                switch (ch.ni * 8 + ch.mode) {
                    case 4 * 8 + 0: return x64(Int<4>{}, Int<0>{});
                    case 5 * 8 + 0: return x64(Int<5>{}, Int<0>{});
                    case 4 * 8 + 1: return x64(Int<4>{}, Int<1>{});
                    case 5 * 8 + 1: return x64(Int<5>{}, Int<1>{});
                    case 4 * 8 + 2: return x64(Int<4>{}, Int<2>{});
                    case 5 * 8 + 2: return x64(Int<5>{}, Int<2>{});
                    case 4 * 8 + 3: return x64(Int<4>{}, Int<3>{});
                    case 5 * 8 + 7: return x64(Int<5>{}, Int<7>{});
                    case 5 * 8 + 3: return x64(Int<5>{}, Int<3>{});
                }
                return hipErrorInvalidValue;
            case GemmKernel::X64P: return launch_gemm_x64p<PR>(A, B, C, bias, M, N, K, out_f32, gelu, accumulate, opts.ld, opts.gelu_form, s);
            case GemmKernel::W4X: return launch_gemm_w4x<PR>(A, B, C, bias, M, N, K, out_f32, gelu, accumulate, opts.ld, opts.gelu_form, s);
            case GemmKernel::K256: return gemm_fam::k256(prec, A, B, C, bias, add2d, add2d_period, M, N, s);
#ifdef SAMRS_EXPERIMENTS
            case GemmKernel::M32: return gemm_fam::m32(prec, ch.mode ? 1 : 0, A, B, C, bias, M, N, K, out_f32, gelu, accumulate, ch.persistent, s);
            case GemmKernel::W4: return gemm_fam::w4(prec, A, B, C, bias, M, N, K, out_f32, gelu, accumulate, ch.persistent, s);
            case GemmKernel::ABL_BIG:
            case GemmKernel::ABL_X64: return launch_gemm_abl(ch, A, B, C, bias, add2d, add2d_period, M, N, K, s);
#else
            default: break;      // the rule picks the experiment kernels in a build that has them only
#endif
        }
        return hipErrorInvalidValue;
    });
}

bool gemm_has_experiments() {
#ifdef SAMRS_EXPERIMENTS
    return true;
#else
    return false;
#endif
}
#ifdef SAMRS_EXPERIMENTS
hipError_t gemm_fam::x64p_fold(int prec, const void* A, const void* B, void* C, const float* bias, const float* cvec, const float* rowstat,
                               int M, int N, int K, bool gelu, hipStream_t s) {
    return with_prec(prec, [&](auto P) { return launch_gemm_x64p_fold<P.value>(A, B, C, bias, cvec, rowstat, M, N, K, gelu, s); });
}
#endif

// One-launch split product (see seg_src_a): C = (A + A_lo)(B + B_lo)^T minus the lo x lo term, + bias; ET output (rounded once
// from the fp32 accumulators) or fp32 output, optionally accumulated into C.  Shapes of the pair-stage 256x320 tile only; the
// caller falls back to three accumulating launch_gemm_et passes when this returns hipErrorInvalidValue.
template <int PREC>
static hipError_t launch_gemm_split3_prec(const uint16_t* a, const uint16_t* al, const uint16_t* b, const uint16_t* bl, void* C,
                                          const float* bias, int M, int N, int K, bool out_f32, bool accumulate, int split_from_n,
                                          const float* add2d, int add2d_period, hipStream_t s) {
    if (out_f32) {
        // fp32 outputs: one tile per block; 256 x 320 tiles where N allows, else 256 x 256 (the neck: N = 256)
        if (N % WBN == 0)
            gemm_et_x64_kernel<PREC, true, false, 5, 3, 0, true><<<dim3((M / QBM) * (N / WBN)), dim3(QTHREADS), 0, s>>>(
                a, b, C, bias, add2d, add2d_period, M, N, K, accumulate ? 1 : 0, 0, al, bl);
        else
            gemm_et_x64_kernel<PREC, true, false, 4, 3, 0, true><<<dim3((M / QBM) * (N / QBN)), dim3(QTHREADS), 0, s>>>(
                a, b, C, bias, add2d, add2d_period, M, N, K, accumulate ? 1 : 0, 0, al, bl);
    } else {
        const int ntiles = (M / QBM) * (N / WBN);
        const int n_cu = cu_count_now();
        gemm_et_x64p_kernel<PREC, false, false, false, true><<<dim3(ntiles < n_cu ? ntiles : n_cu), dim3(QTHREADS), 0, s>>>(
            a, b, C, bias, M, N, K, 0, nullptr, nullptr, al, bl, split_from_n);
    }
    return hipGetLastError();
}

bool gemm_split3_ok(int M, int N, int K, bool out_f32) {
    return M > 0 && N > 0 && K > 0 && M % QBM == 0 && K % XBK == 0 && (N % WBN == 0 || (out_f32 && N % QBN == 0));
}

hipError_t launch_gemm_et_split3(int prec, const void* A, const void* A_lo, const void* B, const void* B_lo, void* C, const float* bias,
                                 int M, int N, int K, bool out_f32, bool accumulate, hipStream_t s, int split_from_n,
                                 const float* add2d, int add2d_period) {
    if (!gemm_split3_ok(M, N, K, out_f32) || !A || !A_lo || !B || !B_lo || (accumulate && !out_f32)) return hipErrorInvalidValue;
    if (split_from_n < 0 || split_from_n % WBN || (split_from_n && out_f32)) return hipErrorInvalidValue;   // whole tiles; ET outputs only
    if (add2d && (!out_f32 || add2d_period <= 0)) return hipErrorInvalidValue;                              // the fp32 epilogue adds it
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* al = reinterpret_cast<const uint16_t*>(A_lo);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    const uint16_t* bl = reinterpret_cast<const uint16_t*>(B_lo);
    return with_prec(prec, [&](auto P) {
        return launch_gemm_split3_prec<P.value>(a, al, b, bl, C, bias, M, N, K, out_f32, accumulate, split_from_n, add2d, add2d_period, s);
    });
}

// C (fp32) += A B^T + bias, then out_et = LayerNorm(C rows) * gamma + beta in the operand type, by the LayerNorm tail of the 256 x 320
// pair-stage kernel (gemm_et_x64_kernel<LNT>).  Only where that kernel is what launch_gemm_et would pick for the shape anyway (fp32
// output with at least one full round of 256 x 320 tiles) and N is one LayerNorm row; otherwise hipErrorInvalidValue and the caller
// launches GEMM and LayerNorm separately.  counters: M / 256 zeroed uint32 (left zero by every launch).
hipError_t launch_gemm_et_lntail(int prec, const void* A, const void* B, float* C, const float* bias, int M, int N, int K,
                                 const float* gamma, const float* beta, float eps, void* out_et, unsigned int* counters, hipStream_t s) {
    if (!gemm_lntail_ok(M, N, K) || !A || !B || !C || !gamma || !beta || !out_et || !counters) return hipErrorInvalidValue;
    LnTail ln;
    ln.gamma = gamma; ln.beta = beta; ln.out = reinterpret_cast<uint16_t*>(out_et); ln.counters = counters; ln.eps = eps;
    dim3 grid((M / QBM) * (N / WBN)), block(QTHREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    return with_prec(prec, [&](auto P) {
        gemm_et_x64_kernel<P.value, true, false, 5, 3, 0, false, true><<<grid, block, 0, s>>>(a, b, C, bias, nullptr, 1, M, N, K, 1, g_x64_skew, nullptr, nullptr, ln);
        return hipGetLastError();
    });
}

void set_gemm_variant(int v) { g_gemm_variant = v; }
int swap_gemm_variant_override(int v) { const int old = tl_gemm_variant; tl_gemm_variant = v; return old; }
void set_gemm_skew(int xcd_units, int cu_units) { g_x64_skew = (xcd_units & 0xffff) | (cu_units << 16); }


// ---- MXFP4 lo-term GEMM (gemm_et_mx_kernel) ----------------------------------------------------------------------------------
bool gemm_mx_ok(int M, int N, int K, int Kp) {
    return M > 0 && N > 0 && K > 0 && M % QBM == 0 && N % WBN == 0 && K % XBK == 0 && Kp > 0 && Kp % MXK == 0;
}
size_t mx_scale_bytes(int rows, int Kp, bool is_b) {
    return is_b ? (size_t)((rows + 319) / 320) * (Kp / MXK) * MX_SB_BYTES : (size_t)((rows + 255) / 256) * (Kp / MXK) * MX_SA_BYTES;
}
hipError_t launch_gemm_et_mx(int prec, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, int Kp,
                             const void* a4_lo, const void* a4_hi, const void* sa_lo, const void* sa_hi,
                             const void* b4_hi, const void* b4_lo, const void* sb_hi, const void* sb_lo,
                             bool out_f32, bool accumulate, int split_from_n, hipStream_t s, bool gelu, void* o4_hi, void* o4_lo,
                             void* so_hi, void* so_lo, int ld, bool ext) {
    if ((gelu || o4_hi) && out_f32) return hipErrorInvalidValue;
    if (ld < 0 || (ld && ld < K + (ext ? XBK : 0)) || (ext && (!ld || o4_hi || out_f32 || split_from_n <= 0))) return hipErrorInvalidValue;
    // the MX-row epilogue goes with lo terms on every tile or (split_from_n == N) on none
    if (o4_hi && (!o4_lo || !so_hi || !so_lo || N % 80 || ((N / 80) * 96) % MXK || (split_from_n && split_from_n != N))) return hipErrorInvalidValue;
    if (!gemm_mx_ok(M, N, K, Kp) || !A || !B || !C || !a4_lo || !a4_hi || !sa_lo || !sa_hi || !b4_hi || !b4_lo || !sb_hi || !sb_lo)
        return hipErrorInvalidValue;
    if ((accumulate && !out_f32) || split_from_n < 0 || split_from_n % WBN || (split_from_n && out_f32)) return hipErrorInvalidValue;
    // no tile takes lo terms and the output is wanted as MX rows (lin1 of split 207): the plain persistent kernel with the MX-row
    // epilogue -- the f16 main loop of gemm_et_x64p_kernel is ~5 % faster than this kernel's (SAMRS_MX_LIN1=0: A/B switch)
    static const bool x64p_lin1 = [] { const char* v = getenv("SAMRS_MX_LIN1"); return !(v && atoi(v) == 0); }();
    if (x64p_lin1 && o4_hi && split_from_n == N && N % XBK == 0 && K % XBK == 0) {
        return with_prec(prec, [&](auto P) { return launch_gemm_x64p_mxo<P.value>(A, B, C, bias, M, N, K, gelu, o4_hi, o4_lo, so_hi, so_lo, s); });
    }
    MxOperands mx;
    mx.a4_lo = (const unsigned char*)a4_lo; mx.a4_hi = (const unsigned char*)a4_hi;
    mx.b4_hi = (const unsigned char*)b4_hi; mx.b4_lo = (const unsigned char*)b4_lo;
    mx.sa_lo = (const unsigned char*)sa_lo; mx.sa_hi = (const unsigned char*)sa_hi;
    mx.sb_hi = (const unsigned char*)sb_hi; mx.sb_lo = (const unsigned char*)sb_lo;
    mx.Kp = Kp; mx.split_from_n = split_from_n;
    const int ntiles = (M / QBM) * (N / WBN);
    static const bool one_tile = [] { const char* v = getenv("SAMRS_MX_PERSIST"); return v && atoi(v) == 0; }();   // 0: one block per tile (A/B runs)
    const int n_cu = one_tile ? 1 << 30 : cu_count();
    const dim3 grid(ntiles < n_cu ? ntiles : n_cu), block(QTHREADS);
    const uint16_t* a = reinterpret_cast<const uint16_t*>(A);
    const uint16_t* b = reinterpret_cast<const uint16_t*>(B);
    const int acc = accumulate ? 1 : 0;
    MxOut mxo;
    mxo.q_hi = (unsigned char*)o4_hi; mxo.q_lo = (unsigned char*)o4_lo; mxo.s_hi = (unsigned char*)so_hi; mxo.s_lo = (unsigned char*)so_lo;
    return with_prec(prec, [&](auto P) {
        constexpr int PR = P.value;
        if (out_f32) gemm_et_mx_kernel<PR, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc, mx, MxOut(), ld, ext ? 1 : 0);
        else if (o4_hi && gelu) gemm_et_mx_kernel<PR, false, true, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc, mx, mxo, ld, ext ? 1 : 0);
        else if (o4_hi) gemm_et_mx_kernel<PR, false, false, true><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc, mx, mxo, ld, ext ? 1 : 0);
        else if (gelu) gemm_et_mx_kernel<PR, false, true, false><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc, mx, MxOut(), ld, ext ? 1 : 0);
        else gemm_et_mx_kernel<PR, false><<<grid, block, 0, s>>>(a, b, C, bias, M, N, K, acc, mx, MxOut(), ld, ext ? 1 : 0);
        return hipGetLastError();
    });
}

// fp32 [rows][K] (x) or the ET pair (hi_in, lo_in) -> fp4 hi / lo [rows][Kp / 2] + their scale tiles; Kp = K / G * GP
hipError_t launch_mx4_pack(int prec, const float* x, const void* hi_in, const void* lo_in, void* out_hi, void* q_hi, void* q_lo,
                           void* s_hi, void* s_lo, int rows, int K, int G, int GP, bool is_b, hipStream_t s, int perm) {
    if (rows <= 0 || K <= 0 || G <= 0 || K % G || G % 4 || GP % 32 || GP < G || ((K / G) * GP) % MXK) return hipErrorInvalidValue;
    if (!x && !(hi_in && lo_in)) return hipErrorInvalidValue;
    const long items = (long)rows * ((K / G) * GP / 32);
    const dim3 grid((unsigned)((items * 8 + 255) / 256)), block(256);
    const uint16_t* hi = reinterpret_cast<const uint16_t*>(hi_in);
    const uint16_t* lo = reinterpret_cast<const uint16_t*>(lo_in);
    return with_prec(prec, [&](auto P) {
        auto pack = [&](auto SRC_F32) {
            mx4_pack_kernel<P.value, SRC_F32.value><<<grid, block, 0, s>>>(x, hi, lo, (uint16_t*)out_hi, (unsigned char*)q_hi, (unsigned char*)q_lo,
                                                                        (unsigned char*)s_hi, (unsigned char*)s_lo, rows, K, G, GP, is_b ? 1 : 0, perm);
        };
        if (x) pack(std::true_type{}); else pack(std::false_type{});
        return hipGetLastError();
    });
}
