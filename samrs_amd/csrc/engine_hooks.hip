// engine_hooks.hip -- the test and tool hooks of include/samrs_hip_internal.h: one kernel or launcher each (samrs_k_*) and the reads of
// engine internals (samrs_debug_*).  Not part of the product path; samrs_debug_encoder_prefix sits in engine_encode.hip with the pass it cuts short.
#include <mutex>

#include "engine_state.h"

extern "C" {
void samrs_debug_set_gemm_variant(int v) { set_gemm_variant(v); }
void samrs_debug_gemm_choice(int prec, int M, int N, int K, int out_f32, int gelu, int accumulate, int has_add2d, int ld, int variant,
                             int32_t* out) {
    gemm_debug_choice(prec, M, N, K, out_f32 != 0, gelu != 0, accumulate != 0, has_add2d != 0, ld, variant, out);
}
void samrs_debug_set_gemm_skew(int xcd_units, int cu_units) { set_gemm_skew(xcd_units, cu_units); }
int samrs_debug_has_experiments(void) { return gemm_has_experiments() ? 1 : 0; }

// test hook: copy (a prefix of) a named internal decoder buffer to a caller device buffer
int samrs_debug_copy_buffer(samrs_engine_t* e, const char* name, void* dst, size_t bytes, void* stream) {
    if (!e || !name || !dst) return SAMRS_ERR_BAD_ARG;
    const std::string n(name);
    const void* src = nullptr;
    if (n == "Q") src = e->Q; else if (n == "TOK0") src = e->TOK0; else if (n == "KF") src = e->KF; else if (n == "KE") src = e->KE;
    else if (n == "KVQ") src = e->KVQ; else if (n == "OI") src = e->OI; else if (n == "U1raw") src = e->U1raw;
    else if (n == "U1") src = e->U1; else if (n == "U2") src = e->U2; else if (n == "HYPER") src = e->HYPER;
    else if (n == "K0F") src = e->K0F; else if (n == "K0E") src = e->K0E; else if (n == "O128") src = e->O128;
    else if (n == "MH") src = e->MH; else if (n == "KT") src = e->KT; else if (n == "VT") src = e->VT; else if (n == "QP") src = e->QP;
    else if (n == "DENSE") src = e->DENSE;      // allocated by the first mask prompt
    else return fail(e, SAMRS_ERR_BAD_ARG, "unknown buffer %s", name);
    // every other name is allocated by samrs_finalize_weights: null before it
    if (!src) return fail(e, SAMRS_ERR_BAD_ARG, "buffer %s is not allocated yet", name);
    CK(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SAMRS_OK;
}

int samrs_debug_time_dominant_kernel(samrs_engine_t* e, int enable) {
    if (!e) return SAMRS_ERR_BAD_ARG;
    e->timing = enable != 0;
    return SAMRS_OK;
}

int samrs_debug_dominant_kernel_time(samrs_engine_t* e, float* avg_ms, int* launches, int* M, int* N, int* K) {
    if (!e || !avg_ms || !launches) return SAMRS_ERR_BAD_ARG;
    double tot = 0.0;
    int n = 0;
    for (auto& pr : e->tev) {
        CK(e, hipEventSynchronize(pr.second));
        float ms = 0.f;
        CK(e, hipEventElapsedTime(&ms, pr.first, pr.second));
        tot += ms;
        ++n;
        e->tpool.push_back(pr.first);
        e->tpool.push_back(pr.second);
    }
    e->tev.clear();
    *avg_ms = n ? (float)(tot / n) : 0.f;
    *launches = n;
    if (M) *M = 0;   // rows vary with the batch of each call; the caller knows its batch
    if (N) *N = 4 * e->D;
    if (K) *K = e->D;
    return SAMRS_OK;
}

// ---- kernel-level entry points -------------------------------------------------------------------
int samrs_k_gemm(int prec, const void* A, const void* B, void* C, const float* bias, const float* add2d, int period,
                 int M, int N, int K, int out_f32, int gelu, int accumulate, void* stream) {
    KRET(launch_gemm_et(prec, A, B, C, bias, add2d, period, M, N, K, out_f32 != 0, gelu != 0, accumulate != 0, (hipStream_t)stream));
}
int samrs_k_gemm_stats(int prec, const void* A, const void* B, float* C, const float* bias, void* xh, float* stats, int M, int N,
                       int K, void* stream) {
    KRET(launch_gemm_et_stats(prec, A, B, C, bias, xh, stats, M, N, K, (hipStream_t)stream));
}
int samrs_k_gemm_fold(int prec, const void* xh, const void* Wf, void* C, const float* bias_f, const float* cvec, const float* rowstat,
                      int M, int N, int K, int gelu, void* stream) {
    KRET(launch_gemm_et_fold(prec, xh, Wf, C, bias_f, cvec, rowstat, M, N, K, gelu != 0, (hipStream_t)stream));
}
int samrs_k_ln_rowstat(const float* stats, float* rowstat, int rows, float eps, void* stream) {
    KRET(launch_ln_rowstat(stats, rowstat, rows, eps, (hipStream_t)stream));
}
int samrs_k_ln_fold_weight(int prec, const float* W, const float* gamma, const float* beta, const float* bias, void* Wf, float* cvec,
                           float* bias_f, int N, int K, void* stream) {
    KRET(launch_ln_fold_weight(prec, W, gamma, beta, bias, Wf, cvec, bias_f, N, K, (hipStream_t)stream));
}
int samrs_k_rowstats_convert(int prec, const float* X, void* xh, float* stats, int rows, int D, void* stream) {
    KRET(launch_rowstats_convert(prec, X, xh, stats, rows, D, (hipStream_t)stream));
}
int samrs_k_gemm_f32(const float* A, int lda, const float* Wt, const float* bias, float* C, int ldc, int M, int N, int K,
                     int relu, int accumulate, void* stream) {
    KRET(launch_gemm_f32(A, lda, Wt, bias, C, ldc, M, N, K, relu != 0, accumulate != 0, (hipStream_t)stream));
}
int samrs_k_convert(int prec, const float* in, void* out, int64_t n, void* stream) {
    KRET(launch_convert(prec, in, out, (long)n, (hipStream_t)stream));
}
int samrs_k_layernorm(int prec, const float* X, const float* gamma, const float* beta, float eps, void* out_et,
                      float* out_f32, int rows_out, int D, int window_mode, int n_images, int grid, int window, void* stream) {
    (void)n_images;
    KRET(launch_layernorm(prec, X, gamma, beta, eps, out_et, out_f32, rows_out, D, window_mode, grid, window, (hipStream_t)stream));
}
int samrs_k_layernorm_mx(int prec, const float* X, const float* gamma, const float* beta, float eps, void* out_et, int rows, int D,
                         void* q_hi, void* q_lo, void* s_hi, void* s_lo, void* stream) {
    KRET(launch_layernorm(prec, X, gamma, beta, eps, out_et, nullptr, rows, D, 0, 0, 0, (hipStream_t)stream, nullptr, q_hi, q_lo, s_hi, s_lo));
}
int samrs_k_window_attention(int prec, const void* qkv, const float* qkv_bias, const float* rel_h, const float* rel_w, void* out,
                             int n_images, int grid, int window, int heads, int head_dim, void* stream) {
    KRET(launch_window_attention(prec, qkv, qkv_bias, rel_h, rel_w, out, n_images, grid, window, heads, head_dim, (hipStream_t)stream));
}
// test hook: the windowed kernel with its split remainder and the per-head mask of out_lo that the engine sets from EncBlock::oc_heads
int samrs_k_window_attention_lo(int prec, const void* qkv, const float* qkv_bias, const float* rel_h, const float* rel_w, void* out,
                                void* out_lo, int n_images, int grid, int heads, int head_dim, uint32_t lo_heads, void* stream) {
    KRET(launch_window_attention(prec, qkv, qkv_bias, rel_h, rel_w, out, n_images, grid, 14, heads, head_dim, (hipStream_t)stream, out_lo,
                                 nullptr, nullptr, nullptr, nullptr, lo_heads));
}
// V^T workspace of the two global-attention TEST / BENCH hooks below (the engine owns its own: e->VTG).  One grow-only buffer per
// DEVICE, looked up under a lock.  A buffer that is outgrown is RETIRED, never freed: another thread of the same device may hold the
// old pointer between this function's return and its own kernel launch (the pointer leaves the lock), and a device synchronisation
// only covers launches that are already enqueued.  Buffers at least double, so the retired ones sum to less than the live
// one; these entry points exist for tests/ and tools/ only (samrs_hip_internal.h says so).
static void* kernel_hook_workspace(size_t need) {
    static std::mutex mu;
    static std::map<int, std::pair<void*, size_t>> per_dev;
    static std::vector<void*> retired;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    auto& w = per_dev[dev];
    if (need > w.second) {
        const size_t want = need > 2 * w.second ? need : 2 * w.second;
        void* p = nullptr;
        if (hipMalloc(&p, want) != hipSuccess) return nullptr;
        if (w.first) retired.push_back(w.first);
        w = {p, want};
    }
    return w.first;
}
int samrs_k_global_attention(int prec, const void* qkv, const float* rel_h, const float* rel_w, void* out, int n_images,
                             int grid, int heads, int head_dim, void* stream) {
    // test / bench hook: the V^T workspace the engine owns is a grow-only static here
    const size_t need = (size_t)n_images * heads * head_dim * grid * grid * 2;
    void* ws = kernel_hook_workspace(need);
    if (!ws) return SAMRS_ERR_HIP;
    KRET(launch_global_attention(prec, qkv, rel_h, rel_w, out, n_images, grid, heads, head_dim, ws, (hipStream_t)stream));
}
int samrs_k_attention_mx(int prec, int global, const void* qkv, const float* qkv_bias, const float* rel_h, const float* rel_w, void* out,
                         void* out_lo, int n_images, int grid, int heads, int head_dim, void* q_hi, void* q_lo, void* s_hi, void* s_lo,
                         void* stream) {
    if (!global)
        KRET(launch_window_attention(prec, qkv, qkv_bias, rel_h, rel_w, out, n_images, grid, 14, heads, head_dim, (hipStream_t)stream, out_lo,
                                     q_hi, q_lo, s_hi, s_lo));
    const size_t need = (size_t)n_images * heads * head_dim * grid * grid * 2;
    void* ws = kernel_hook_workspace(need);
    if (!ws) return SAMRS_ERR_HIP;
    KRET(launch_global_attention(prec, qkv, rel_h, rel_w, out, n_images, grid, heads, head_dim, ws, (hipStream_t)stream, out_lo, q_hi, q_lo, s_hi, s_lo));
}
// test hook: the outlier K-columns picked for block GEMM `gemm` (0 qkv, 1 lin1, 2 lin2, 3 proj) of encoder block `block`; returns the count
// (<= 32) and copies the indices (ascending) to the HOST array `out32`, or a negative status
int samrs_debug_outlier_columns(samrs_engine_t* e, int block, int gemm, int32_t* out32) {
    if (!e || !out32 || gemm < 0 || gemm > 3 || block < 0 || block >= (int)e->blocks.size()) return SAMRS_ERR_BAD_ARG;
    const EncBlock& b = e->blocks[block];
    if (b.oc_n[gemm] > 0) {
        ON_DEVICE(e);
        CK(e, hipMemcpy(out32, b.oc_idx[gemm], sizeof(int32_t) * b.oc_n[gemm], hipMemcpyDeviceToHost));
    }
    return b.oc_n[gemm];
}
int samrs_k_range_profile(int prec, const void* x, long n, int cols, int ld, int64_t* row48, void* stream) {
    if (!x || !row48 || n < 0) return SAMRS_ERR_BAD_ARG;
    KRET(launch_range_profile(prec, x, n, cols, ld, reinterpret_cast<long long*>(row48), (hipStream_t)stream));
}
int samrs_k_column_stats(int prec, const void* x, int M, int K, int ld, float* partials, double* sumsq, uint32_t* maxbits, void* stream) {
    if (!x || !partials || !sumsq || !maxbits) return SAMRS_ERR_BAD_ARG;
    KRET(launch_column_stats(prec, x, M, K, ld, partials, sumsq, maxbits, (hipStream_t)stream));
}
int samrs_k_audit_rows_per_partial(void) { return AUDIT_ROWS_PER_PARTIAL; }
// ---- the outlier-column kernels and the padded-row / EXT-stage GEMM launches, one each (tests/test_outlier_kernels_gpu.py).  The engine
// builds its column lists itself (engine.hip pick_outlier_columns: distinct, ascending, below the column count) and sizes every buffer from
// its own shapes; a caller of these hooks does neither, so each repeats those guarantees on the host before anything is launched.
// idx_ok: n <= 32 device indices, read back on `stream`, are distinct, ascending and below `bound` (n == 0: nothing to read).
static bool idx_ok(const int32_t* idx, int n, int bound, void* stream) {
    if (n == 0) return true;
    int32_t h[32];
    if (!idx || n < 0 || n > 32 || bound < 1) return false;
    if (hipMemcpyAsync(h, idx, sizeof(int32_t) * n, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess) return false;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return false;
    for (int j = 0; j < n; ++j)
        if (h[j] < 0 || h[j] >= bound || (j && h[j] <= h[j - 1])) return false;
    return true;
}
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int samrs_k_gemm_ld(int prec, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, int ld, int gelu, int gelu_form,
                    void* stream) {
    if (!A || !B || !C || !aligned16(A) || !aligned16(B) || !aligned16(C)) return SAMRS_ERR_BAD_ARG;
    if (ld < 0 || (gelu_form != 1 && gelu_form != 2)) return SAMRS_ERR_BAD_ARG;
    GemmOpts opts;
    opts.ld = ld;
    opts.gelu_form = gelu_form;
    KRET(launch_gemm_et(prec, A, B, C, bias, nullptr, 0, M, N, K, false, gelu != 0, false, (hipStream_t)stream, opts));
}
int samrs_k_gemm_ext(int prec, const void* A, const void* B, const void* Ax, const void* Bx, float* C, const float* bias, int M, int N, int K,
                     void* stream) {
    if (!A || !B || !Ax || !Bx || !C || !aligned16(A) || !aligned16(B) || !aligned16(Ax) || !aligned16(Bx) || !aligned16(C)) return SAMRS_ERR_BAD_ARG;
    if (M < 1 || N < 1 || K < 1 || !gemm_ext_ok(M, N, K)) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_gemm_et_ext(prec, A, B, Ax, Bx, C, bias, M, N, K, (hipStream_t)stream));
}
int samrs_k_layernorm_ext(int prec, const float* X, const float* gamma, const float* beta, float eps, void* out_et, int rows, int D, int ld_out,
                          const int32_t* oc_idx, int n_oc, int window_mode, void* stream) {
    if (!X || !gamma || !beta || !out_et || !aligned16(X) || !aligned16(gamma) || !aligned16(beta) || !aligned16(out_et)) return SAMRS_ERR_BAD_ARG;
    if (rows < 1 || D < 4 || ld_out < 0 || n_oc < 0 || n_oc > 32 || (n_oc && ld_out < D + 64)) return SAMRS_ERR_BAD_SHAPE;
    if (window_mode) return SAMRS_ERR_BAD_SHAPE;       // the extension goes with plain row order only, and the hook has no grid to give
    if (!idx_ok(oc_idx, n_oc, D, stream)) return SAMRS_ERR_BAD_ARG;
    KRET(launch_layernorm(prec, X, gamma, beta, eps, out_et, nullptr, rows, D, 0, 0, 0, (hipStream_t)stream, nullptr, nullptr, nullptr, nullptr,
                          nullptr, ld_out, n_oc ? oc_idx : nullptr, n_oc));
}
int samrs_k_outlier_weight_ext(int prec, const float* W, int N, int K, const int32_t* idx, int n_oc, void* out, int ld, int col0, void* stream) {
    if (!W || !out || N < 1 || K < 1 || n_oc < 0 || n_oc > 32 || col0 < 0 || ld < col0 + 64) return SAMRS_ERR_BAD_SHAPE;
    if (!idx_ok(idx, n_oc, K, stream)) return SAMRS_ERR_BAD_ARG;
    KRET(launch_outlier_weight_ext(prec, W, N, K, idx, n_oc, out, ld, col0, (hipStream_t)stream));
}
// n_rows1: the rows of W1 (lin1's output width), which the launcher does not need and the check of idx2 does
int samrs_k_outlier_side_weight(int prec, const float* W1, const float* b1, int n_rows1, int D, const int32_t* idx2, int n2, const int32_t* idx1,
                                int n1, void* out, int Ks, float* bias_out, void* stream) {
    if (!W1 || !b1 || !out || n_rows1 < 1 || D < 1 || n2 < 1 || n2 > 32 || n1 < 0 || n1 > 32 || Ks < D + (n1 ? 64 : 0)) return SAMRS_ERR_BAD_SHAPE;
    if (!idx_ok(idx2, n2, n_rows1, stream) || !idx_ok(idx1, n1, D, stream)) return SAMRS_ERR_BAD_ARG;
    KRET(launch_outlier_side_weight(prec, W1, b1, D, idx2, n2, idx1, n1, out, Ks, bias_out, (hipStream_t)stream));
}
int samrs_k_outlier_gather(const void* hi, const void* lo, int D, const int32_t* idx, int n_oc, void* out, int rows, void* stream) {
    if (!hi || !lo || !out || D < 1 || n_oc < 1 || n_oc > 32 || rows < 1) return SAMRS_ERR_BAD_SHAPE;
    if (!idx_ok(idx, n_oc, D, stream)) return SAMRS_ERR_BAD_ARG;
    KRET(launch_outlier_gather(hi, lo, D, idx, n_oc, out, rows, (hipStream_t)stream));
}
int samrs_k_outlier_side_gemm(int prec, const void* Y, int lda, const void* Ws, const float* bias, int M, int K, void* out, void* stream) {
    if (!Y || !Ws || !bias || !out || !aligned16(Y) || !aligned16(Ws)) return SAMRS_ERR_BAD_ARG;
    if (M < 64 || M % 64 || K < 32 || K % 32 || lda < K || lda % 8) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_outlier_side_gemm(prec, Y, lda, Ws, bias, M, K, out, (hipStream_t)stream));
}
int samrs_k_weight_norms(const float* W, int N, int K, float* col_sq, float* row_sq, void* stream) {
    if (!W || (!col_sq && !row_sq)) return SAMRS_ERR_BAD_ARG;
    if (N < 1 || K < 1) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_weight_norms(W, N, K, col_sq, row_sq, (hipStream_t)stream));
}
int samrs_k_range_scan(int prec, const void* x, int64_t n, int cols, int ld, uint64_t* counter, void* stream) {
    if (!x || !counter || !aligned16(x)) return SAMRS_ERR_BAD_ARG;
    if (n < 0 || n % 8 || (cols > 0 && (cols % 8 || ld % 8 || ld < cols || n % cols))) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_range_scan(prec, x, (long)n, reinterpret_cast<unsigned long long*>(counter), (hipStream_t)stream, cols, ld));
}
int samrs_k_neck_im2col(const void* in, void* A, int n_images, int grid, int C, void* stream) {
    if (!in || !A || n_images < 1 || grid < 1 || C < 8 || C % 8) return SAMRS_ERR_BAD_ARG;
    KRET(launch_neck_im2col(in, A, n_images, grid, C, (hipStream_t)stream));
}
// ---- the token-side fp32 GEMM batch, image ingest, embedding hand-over and reference-grade GELU, one kernel each
// (tests/test_token_side_kernels_gpu.py).  The engine fills an F32Batch from its own buffers (hipMalloc: 256-byte aligned; row strides
// C, Ci, T C, 2048: multiples of 4 floats no shorter than K; weights dense [N][K] with K % 16 == 0, a row offset into them whole rows) and
// sizes every output from its own shapes; a caller of these hooks does neither, so each repeats that on the host before anything is launched.
int samrs_k_gemm_f32_batch(const float* const* A, const float* const* A2, const float* const* W, const float* const* bias, float* const* C,
                           int count, int lda, int ldc, int M, int N, int K, int relu, int accumulate, void* stream) {
    if (!A || !W || !bias || !C || count < 1 || count > F32_BATCH_MAX) return SAMRS_ERR_BAD_ARG;
    if (M < 1 || N < 1 || K < 16 || K % 16 || lda % 4 || lda < K || ldc < N) return SAMRS_ERR_BAD_ARG;
    F32Batch bt{};
    for (int z = 0; z < count; ++z) {
        const float* a2 = A2 ? A2[z] : nullptr;
        if (!A[z] || !W[z] || !C[z] || !aligned16(A[z]) || !aligned16(a2) || !aligned16(W[z])) return SAMRS_ERR_BAD_ARG;      // the kernel reads float4
        bt.A[z] = A[z]; bt.A2[z] = a2; bt.W[z] = W[z]; bt.bias[z] = bias[z]; bt.C[z] = C[z];
    }
    KRET(launch_gemm_f32_batch(bt, count, lda, ldc, M, N, K, relu != 0, accumulate != 0, (hipStream_t)stream));
}
int samrs_k_patch_im2col(int prec, const uint8_t* img_u8, void* A_et, void* A_lo_et /* may be null */, int n_images, int in_h, int in_w,
                         int grid, int patch, void* stream) {
    if (!img_u8 || !A_et || !aligned16(A_et) || !aligned16(A_lo_et)) return SAMRS_ERR_BAD_ARG;
    if (patch < 8 || patch % 8 || in_h < 1 || in_w < 1 || n_images < 1 || grid < 1) return SAMRS_ERR_BAD_ARG;
    KRET(launch_patch_im2col(prec, img_u8, A_et, n_images, in_h, in_w, grid, patch, (hipStream_t)stream, A_lo_et));
}
int samrs_k_transpose_f32(const float* in, float* out, int rows, int cols, void* stream) {
    if (!in || !out || rows < 1 || cols < 1) return SAMRS_ERR_BAD_ARG;
    KRET(launch_transpose_f32(in, out, rows, cols, (hipStream_t)stream));
}
int samrs_k_gelu_split(int prec, const float* in, void* hi_et, void* lo_et, int64_t n, void* stream) {
    if (!in || !hi_et || !lo_et || !aligned16(in) || !aligned16(hi_et) || !aligned16(lo_et) || n < 4 || n % 4) return SAMRS_ERR_BAD_ARG;
    KRET(launch_gelu_split(prec, in, hi_et, lo_et, (long)n, (hipStream_t)stream));
}
int samrs_k_postprocess(const float* low, int n_masks, int in_h, int in_w, int orig_h, int orig_w, int img_size,
                        int return_logits, void* out, void* stream) {
    KRET(launch_postprocess(low, n_masks, in_h, in_w, orig_h, orig_w, img_size, return_logits, out, (hipStream_t)stream));
}
int samrs_k_region_labels(const uint8_t* masks, int n, int h, int w, int complement, int32_t* labels_out, void* stream) {
    KRET(launch_region_labels(masks, n, h, w, complement, labels_out, (hipStream_t)stream));
}
int samrs_k_mask_row_extents(const uint8_t* masks, int n, int h, int w, int32_t* ext_out, void* stream) {
    KRET(launch_mask_row_extents(masks, n, h, w, ext_out, (hipStream_t)stream));
}
int samrs_k_mask_hull(const uint8_t* masks, int n, int h, int w, int x0, int y0, int32_t* ext_scratch, int32_t* verts_out, int cap,
                      int32_t* counts_out, void* stream) {
    if (!verts_out || !counts_out || !mask_boxes_shape_ok(h, w, x0, y0)) return SAMRS_ERR_BAD_ARG;
    hipError_t err = launch_mask_row_extents(masks, n, h, w, ext_scratch, (hipStream_t)stream);
    if (err != hipSuccess) KRET(err);
    KRET(launch_mask_hull_rect(ext_scratch, n, h, x0, y0, nullptr, nullptr, nullptr, verts_out, cap, counts_out, (hipStream_t)stream));
}
int64_t samrs_k_polygon_scratch_bytes(int n, int h, int w, int max_edges) {
    if (n < 1 || max_edges < 4 || !mask_polygons_shape_ok(h, w, 0, 0)) return -1;
    return (int64_t)mask_polygons_scratch_bytes(n, h, w, max_edges);
}
int64_t samrs_k_polygon_edge_stride(int h, int w, int max_edges) {
    if (max_edges < 4 || !mask_polygons_shape_ok(h, w, 0, 0)) return -1;
    return (int64_t)mask_polygons_edge_stride(h, w, max_edges);
}
int samrs_k_polygon_edges(const uint8_t* masks, int n, int h, int w, int max_edges, void* scratch, uint32_t* ids_out, int32_t* succ_out,
                          uint8_t* corner_out, int32_t* counts_out, void* stream) {
    KRET(launch_polygon_edges(masks, n, h, w, max_edges, scratch, ids_out, succ_out, corner_out, counts_out, (hipStream_t)stream));
}
int samrs_k_polygon_ranks(const uint8_t* masks, int n, int h, int w, int max_edges, void* scratch, int32_t* leader_out, int32_t* rank_out,
                          int32_t* counts_out, void* stream) {
    KRET(launch_polygon_ranks(masks, n, h, w, max_edges, scratch, leader_out, rank_out, counts_out, (hipStream_t)stream));
}
int64_t samrs_k_polygon_simplify_scratch_bytes(int n, int64_t vertex_capacity, int64_t ring_capacity) {
    if (n < 1 || vertex_capacity < 0 || ring_capacity < 0 || vertex_capacity >= (1ll << 40) || ring_capacity >= (1ll << 40)) return -1;
    return (int64_t)polygon_simplify_scratch_bytes(n, (long long)vertex_capacity, (long long)ring_capacity);
}
int samrs_k_polygon_simplify_keep(const int32_t* vertices, const int32_t* rings, const int64_t* table, int n, int eps_q,
                                  int64_t vertex_capacity, int64_t ring_capacity, void* scratch, uint8_t* keep_out, int32_t* kept_out,
                                  void* stream) {
    KRET(launch_polygon_simplify_keep(vertices, rings, (const long long*)table, n, eps_q, (long long)vertex_capacity,
                                      (long long)ring_capacity, scratch, keep_out, kept_out, (hipStream_t)stream));
}
// ---- the mask upscaler's three entry points (tests/test_upscaler_kernels_gpu.py).  The engine passes its own buffers (hipMalloc: 256-byte
// aligned), prec from its own precision, n >= 1 prompts of a grid that is a multiple of 16, 4 mask tokens with (sel0, n_sel) = (0, 1) or (1, 3)
// and the lo operands all or none (engine_decode.hip); a caller of these hooks guarantees none of that, so each repeats it on the host
// before anything is launched: the kernels read 16-byte pieces, hyper row sel0 + n_sel - 1 of the last prompt must exist, and the
// launchers take any prec other than bf16 as f16 or size their grids from n and grid as they come.
static bool upscaler_prec_ok(int prec) { return prec == PREC_BF16 || prec == PREC_F16; }
static bool upscaler_shape_ok(int n, int grid, int n_mask_tokens, int sel0, int n_sel) {
    if (n < 1 || grid < 16 || grid % 16 || n_mask_tokens < 1 || sel0 < 0 || (n_sel != 1 && n_sel != 3)) return false;
    if (n_sel > n_mask_tokens || sel0 > n_mask_tokens - n_sel) return false;
    return grid <= 1024 && (int64_t)n * grid * grid * 16 <= INT32_MAX;                 // pixel and row counts stay in an int
}
int samrs_k_gemm_gln(int prec, const void* A, const void* B, void* C, const float* bias, const float* gamma_beta, int M, int N,
                     int K, const void* A_lo, const void* B_lo, void* stream) {
    if (!upscaler_prec_ok(prec) || !A || !B || !C || !bias || !gamma_beta || (A_lo == nullptr) != (B_lo == nullptr)) return SAMRS_ERR_BAD_ARG;
    if (!aligned16(A) || !aligned16(B) || !aligned16(C) || !aligned16(bias) || !aligned16(gamma_beta) || !aligned16(A_lo) || !aligned16(B_lo))
        return SAMRS_ERR_BAD_ARG;
    if (M < 256 || M % 256 || N < 128 || N % 128 || K < 32 || K % 32) return SAMRS_ERR_BAD_SHAPE;      // DBM, DBN, DBK of gemm_select.h
    KRET(launch_gemm_et_gln(prec, A, B, C, bias, gamma_beta, M, N, K, (hipStream_t)stream, A_lo, B_lo));
}
int samrs_k_gemm_split3(int prec, const void* A, const void* A_lo, const void* B, const void* B_lo, void* C, const float* bias,
                        int M, int N, int K, int out_f32, int accumulate, int split_from_n, void* stream) {
    if (!gemm_split3_ok(M, N, K, out_f32 != 0)) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_gemm_et_split3(prec, A, A_lo, B, B_lo, C, bias, M, N, K, out_f32 != 0, accumulate != 0, (hipStream_t)stream, split_from_n));
}
int samrs_k_upscale2_masks(int prec, const void* u1, const void* w, const void* w_lo, const float* bias, const float* hyper,
                           float* low, int n, int grid, int n_mask_tokens, int sel0, int n_sel, void* stream) {
    if (!upscaler_prec_ok(prec) || !u1 || !w || !bias || !hyper || !low) return SAMRS_ERR_BAD_ARG;
    if (!aligned16(u1) || !aligned16(w) || !aligned16(w_lo) || !aligned16(bias) || !aligned16(hyper) || !aligned16(low)) return SAMRS_ERR_BAD_ARG;
    if (!upscaler_shape_ok(n, grid, n_mask_tokens, sel0, n_sel)) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_upscale2_masks(prec, u1, w, w_lo, bias, hyper, low, n, grid, n_mask_tokens, sel0, n_sel, (hipStream_t)stream));
}
int samrs_k_upscaler_fused(int prec, const void* keys, const void* keys_lo, const void* w1, const void* w1_lo, const float* b1,
                           const float* ln, const void* w2, const void* w2_lo, const float* b2, const float* hyper, float* low, int n,
                           int grid, int n_mask_tokens, int sel0, int n_sel, void* stream) {
    if (!upscaler_prec_ok(prec) || !keys || !w1 || !b1 || !ln || !w2 || !b2 || !hyper || !low) return SAMRS_ERR_BAD_ARG;
    if ((keys_lo || w1_lo || w2_lo) && !(keys_lo && w1_lo && w2_lo)) return SAMRS_ERR_BAD_ARG;
    if (!aligned16(keys) || !aligned16(keys_lo) || !aligned16(w1) || !aligned16(w1_lo) || !aligned16(b1) || !aligned16(ln) || !aligned16(w2) ||
        !aligned16(w2_lo) || !aligned16(b2) || !aligned16(hyper) || !aligned16(low))
        return SAMRS_ERR_BAD_ARG;
    if (!upscaler_shape_ok(n, grid, n_mask_tokens, sel0, n_sel)) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_upscaler_fused(prec, keys, keys_lo, w1, w1_lo, b1, ln, w2, w2_lo, b2, hyper, low, n, grid, n_mask_tokens, sel0, n_sel,
                               (hipStream_t)stream));
}
int64_t samrs_k_mx_scale_bytes(int rows, int Kp, int is_b) { return (int64_t)mx_scale_bytes(rows, Kp, is_b != 0); }
int samrs_k_mx4_pack(int prec, const float* x, const void* hi_in, const void* lo_in, void* out_hi, void* q_hi, void* q_lo, void* s_hi,
                     void* s_lo, int rows, int K, int G, int GP, int is_b, void* stream) {
    // is_b bit 1: the attention kernels' block-internal element order (launch_mx4_pack perm)
    return launch_mx4_pack(prec, x, hi_in, lo_in, out_hi, q_hi, q_lo, s_hi, s_lo, rows, K, G, GP, (is_b & 1) != 0, (hipStream_t)stream,
                           (is_b & 2) ? 1 : (is_b & 4) ? 2 : 0) == hipSuccess
               ? SAMRS_OK : SAMRS_ERR_BAD_SHAPE;
}
int samrs_k_gemm_mx(int prec, const void* A, const void* B, void* C, const float* bias, int M, int N, int K, int Kp, const void* a4_lo,
                    const void* a4_hi, const void* sa_lo, const void* sa_hi, const void* b4_hi, const void* b4_lo, const void* sb_hi,
                    const void* sb_lo, int out_f32, int accumulate, int split_from_n, void* stream) {
    return launch_gemm_et_mx(prec, A, B, C, bias, M, N, K, Kp, a4_lo, a4_hi, sa_lo, sa_hi, b4_hi, b4_lo, sb_hi, sb_lo, out_f32 != 0,
                             accumulate != 0, split_from_n, (hipStream_t)stream) == hipSuccess ? SAMRS_OK : SAMRS_ERR_BAD_SHAPE;
}
int samrs_k_gemm_mx_gelu_mxout(int prec, const void* A, const void* B, void* C_et, const float* bias, int M, int N, int K, int Kp,
                               const void* a4_lo, const void* a4_hi, const void* sa_lo, const void* sa_hi, const void* b4_hi, const void* b4_lo,
                               const void* sb_hi, const void* sb_lo, int gelu, void* o4_hi, void* o4_lo, void* so_hi, void* so_lo, void* stream) {
    // gelu: bit 0 = GELU in the epilogue, bit 1 = NO tile takes lo terms (split_from_n = N: lin1 of split 207, routed to the persistent
    // plain kernel with the MX-row epilogue)
    return launch_gemm_et_mx(prec, A, B, C_et, bias, M, N, K, Kp, a4_lo, a4_hi, sa_lo, sa_hi, b4_hi, b4_lo, sb_hi, sb_lo, false, false,
                             (gelu & 2) ? N : 0, (hipStream_t)stream, (gelu & 1) != 0, o4_hi, o4_lo, so_hi, so_lo) == hipSuccess
               ? SAMRS_OK : SAMRS_ERR_BAD_SHAPE;
}
int samrs_k_convert_split(int prec, const float* in, void* out_hi, void* out_lo, int64_t n, void* stream) {
    KRET(launch_convert(prec, in, out_hi, (long)n, (hipStream_t)stream, out_lo));
}
// prompt encoder / two-way transformer glue, one kernel each.  The checks in front of a launcher are those the engine's own call
// sites guarantee by construction and the launcher therefore does not repeat; a shape it refuses itself comes back through KRET.
int samrs_k_prompt_tokens(const float* boxes, const float* point_coords, const int32_t* point_labels, int n_prompts, int n_points,
                          float img_size, const float* gauss, const float* point_emb, const float* not_a_point, const float* iou_token,
                          const float* mask_tokens, float* tokens, float* tokens2, int T, void* stream) {
    if (!tokens || !gauss || !point_emb || !not_a_point || !iou_token || !mask_tokens || n_prompts < 1) return SAMRS_ERR_BAD_ARG;
    if ((point_coords != nullptr) != (point_labels != nullptr) || (point_coords && n_points < 1)) return SAMRS_ERR_BAD_ARG;
    PromptParams pp{};
    prompt_call_fields(pp, boxes, point_coords, point_labels, n_prompts, n_points, img_size);
    pp.gauss = gauss;
    for (int i = 0; i < 4; ++i) pp.point_emb[i] = point_emb + i * 256;
    pp.not_a_point = not_a_point; pp.iou_token = iou_token; pp.mask_tokens = mask_tokens;
    if (T != prompt_token_count(boxes != nullptr, pp.n_points)) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_prompt_tokens(pp, tokens, tokens2, T, (hipStream_t)stream));
}
int samrs_k_dense_pe(const float* gauss, float* pe, int grid, void* stream) {
    if (!gauss || !pe || grid < 1) return SAMRS_ERR_BAD_ARG;
    KRET(launch_dense_pe(gauss, pe, grid, (hipStream_t)stream));
}
int samrs_k_mask_embed(const float* w0, const float* b0, const float* ln1w, const float* ln1b, const float* w3, const float* b3,
                       const float* ln4w, const float* ln4b, const float* w6, const float* b6, const float* mask_in, float* dense,
                       int n, int grid, void* stream) {
    if (!mask_in || !dense || n < 1) return SAMRS_ERR_BAD_ARG;
    if (grid < 1 || (grid * grid) % 16) return SAMRS_ERR_BAD_SHAPE;
    const MaskEmbedParams mp{w0, b0, ln1w, ln1b, w3, b3, ln4w, ln4b, w6, b6};
    KRET(launch_mask_embed(mp, mask_in, dense, n, grid, (hipStream_t)stream));
}
int samrs_k_fill_slot_table(const int32_t* start_host, const int32_t* slot_host, int n_runs, int32_t* out, void* stream) {
    if (!start_host || !slot_host || !out || n_runs < 1) return SAMRS_ERR_BAD_ARG;
    KRET(launch_fill_slot_table(start_host, slot_host, n_runs, out, (hipStream_t)stream));
}
int samrs_k_make_keys(int prec, const float* emb, const float* dense, const float* vec, float* out_f32, void* out_et, int n_batches,
                      int tokens, int C, const int32_t* slot_of, void* stream) {
    if (!emb || (!dense && !vec) || !out_f32 || !out_et || n_batches < 1) return SAMRS_ERR_BAD_ARG;
    if (tokens < 1 || C < 4 || C % 4) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_make_keys(prec, emb, dense, vec, out_f32, out_et, n_batches, tokens, C, (hipStream_t)stream, slot_of));
}
int samrs_k_token_self_attn(const float* q, const float* k, const float* v, float* o, int n, int T, int C, int heads, void* stream) {
    if (n < 1 || T < 1 || heads < 1) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_token_self_attn(q, k, v, o, n, T, C, heads, (hipStream_t)stream));
}
int64_t samrs_k_t2i_workspace_floats(int n, int T) { return (int64_t)t2i_workspace_floats(n, T); }
int samrs_k_t2i_attention(int prec, const float* qp, const void* kp, const void* vp, int ld, int64_t bstride, float* out,
                          float* workspace, int n, int T, int tokens, int Ci, int heads, const int32_t* slot_of, void* stream) {
    if (n < 1 || T < 1 || tokens < 1) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_t2i_attention(prec, qp, kp, vp, ld, (long)bstride, out, workspace, n, T, tokens, Ci, heads, (hipStream_t)stream, slot_of));
}
int samrs_k_i2t_attention(int prec, const void* qi, int ld, int64_t bstride, const float* kt, const float* vt, void* out, int n,
                          int T, int tokens, int Ci, int heads, void* stream) {
    if (n < 1 || T < 1 || T > 16 || tokens < 1 || heads < 1) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_i2t_attention(prec, qi, ld, (long)bstride, kt, vt, out, n, T, tokens, Ci, heads, (hipStream_t)stream));
}
int samrs_k_i2t_fused(int prec, const void* qi, int ld, int64_t q_bstride, const float* kt, const float* vt, const void* w,
                      const void* w_lo, const float* bias, const float* resid, int64_t r_bstride, const float* gamma,
                      const float* beta, float eps, float* outF, void* outE, void* outE_lo, int n, int T, int tokens, int Ci, int C,
                      const int32_t* slot_of, void* stream) {
    if (n < 1 || tokens < 1 || !outE || !resid) return SAMRS_ERR_BAD_ARG;
    KRET(launch_i2t_fused(prec, qi, ld, (long)q_bstride, kt, vt, w, w_lo, bias, resid, (long)r_bstride, gamma, beta, eps, outF, outE,
                          outE_lo, n, T, tokens, Ci, C, (hipStream_t)stream, slot_of));
}
int samrs_k_group_ln_gelu(int prec, const float* in, const float* gamma, const float* beta, float eps, void* out, int64_t rows,
                          int groups, int gsize, void* stream) {
    if (rows < 1) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_group_ln_gelu(prec, in, gamma, beta, eps, out, (long)rows, groups, gsize, (hipStream_t)stream));
}
int samrs_k_mask_product(int prec, const void* up2, const float* hyper, float* low, int n, int grid, int n_mask_tokens, int sel0,
                         int n_sel, void* stream) {
    if (n < 1 || grid < 1 || (16 * grid * grid) % 256 || sel0 < 0 || sel0 + n_sel > n_mask_tokens) return SAMRS_ERR_BAD_SHAPE;
    KRET(launch_mask_product(prec, up2, hyper, low, n, grid, n_mask_tokens, sel0, n_sel, (hipStream_t)stream));
}
}  // extern "C"
