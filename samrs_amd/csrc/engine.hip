// engine.hip -- the engine handle of libsamrs_hip.so's C ABI (include/samrs_hip.h): create / destroy, the strict weight contract with
// load-time repacking and every workspace, the per-engine options, the slot flags.  The passes and the other entry points live in
// engine_encode.hip, engine_decode.hip, engine_masks.hip and engine_hooks.hip; engine_state.h is what the five files share.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "engine_state.h"

static int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }

namespace {

bool is_global(const samrs_config& c, int i) {
    for (int k = 0; k < c.n_global; ++k)
        if (c.global_attn_indexes[k] == i) return true;
    return false;
}

// ---- the strict name/shape contract -----------------------------------
void required_tensors(const samrs_engine* e, std::vector<std::pair<std::string, std::vector<int64_t>>>& out) {
    const samrs_config& c = e->cfg;
    const int64_t D = c.embed_dim, g = e->grid, hd = e->hd, C = c.out_chans, P = c.patch_size;
    auto add = [&](const std::string& n, std::vector<int64_t> s) { out.emplace_back(n, std::move(s)); };
    add("image_encoder.pos_embed", {1, g, g, D});
    add("image_encoder.patch_embed.proj.weight", {D, 3, P, P});
    add("image_encoder.patch_embed.proj.bias", {D});
    for (int i = 0; i < c.depth; ++i) {
        const std::string p = "image_encoder.blocks." + std::to_string(i);
        const int64_t s = is_global(c, i) ? g : c.window_size;
        add(p + ".norm1.weight", {D}); add(p + ".norm1.bias", {D});
        add(p + ".attn.rel_pos_h", {2 * s - 1, hd}); add(p + ".attn.rel_pos_w", {2 * s - 1, hd});
        add(p + ".attn.qkv.weight", {3 * D, D}); add(p + ".attn.qkv.bias", {3 * D});
        add(p + ".attn.proj.weight", {D, D}); add(p + ".attn.proj.bias", {D});
        add(p + ".norm2.weight", {D}); add(p + ".norm2.bias", {D});
        add(p + ".mlp.lin1.weight", {4 * D, D}); add(p + ".mlp.lin1.bias", {4 * D});
        add(p + ".mlp.lin2.weight", {D, 4 * D}); add(p + ".mlp.lin2.bias", {D});
    }
    add("image_encoder.neck.0.weight", {C, D, 1, 1});
    add("image_encoder.neck.1.weight", {C}); add("image_encoder.neck.1.bias", {C});
    add("image_encoder.neck.2.weight", {C, C, 3, 3});
    add("image_encoder.neck.3.weight", {C}); add("image_encoder.neck.3.bias", {C});
    add("prompt_encoder.pe_layer.positional_encoding_gaussian_matrix", {2, C / 2});
    for (int i = 0; i < 4; ++i) add("prompt_encoder.point_embeddings." + std::to_string(i) + ".weight", {1, C});
    add("prompt_encoder.not_a_point_embed.weight", {1, C});
    add("prompt_encoder.no_mask_embed.weight", {1, C});
    add("prompt_encoder.mask_downscaling.0.weight", {4, 1, 2, 2}); add("prompt_encoder.mask_downscaling.0.bias", {4});
    add("prompt_encoder.mask_downscaling.1.weight", {4}); add("prompt_encoder.mask_downscaling.1.bias", {4});
    add("prompt_encoder.mask_downscaling.3.weight", {16, 4, 2, 2}); add("prompt_encoder.mask_downscaling.3.bias", {16});
    add("prompt_encoder.mask_downscaling.4.weight", {16}); add("prompt_encoder.mask_downscaling.4.bias", {16});
    add("prompt_encoder.mask_downscaling.6.weight", {C, 16, 1, 1}); add("prompt_encoder.mask_downscaling.6.bias", {C});
    auto attn = [&](const std::string& p, int64_t internal) {
        add(p + ".q_proj.weight", {internal, C}); add(p + ".q_proj.bias", {internal});
        add(p + ".k_proj.weight", {internal, C}); add(p + ".k_proj.bias", {internal});
        add(p + ".v_proj.weight", {internal, C}); add(p + ".v_proj.bias", {internal});
        add(p + ".out_proj.weight", {C, internal}); add(p + ".out_proj.bias", {C});
    };
    for (int i = 0; i < 2; ++i) {
        const std::string p = "mask_decoder.transformer.layers." + std::to_string(i);
        attn(p + ".self_attn", C);
        attn(p + ".cross_attn_token_to_image", C / 2);
        attn(p + ".cross_attn_image_to_token", C / 2);
        for (int k = 1; k <= 4; ++k) {
            add(p + ".norm" + std::to_string(k) + ".weight", {C});
            add(p + ".norm" + std::to_string(k) + ".bias", {C});
        }
        add(p + ".mlp.lin1.weight", {2048, C}); add(p + ".mlp.lin1.bias", {2048});
        add(p + ".mlp.lin2.weight", {C, 2048}); add(p + ".mlp.lin2.bias", {C});
    }
    attn("mask_decoder.transformer.final_attn_token_to_image", C / 2);
    add("mask_decoder.transformer.norm_final_attn.weight", {C}); add("mask_decoder.transformer.norm_final_attn.bias", {C});
    add("mask_decoder.iou_token.weight", {1, C});
    add("mask_decoder.mask_tokens.weight", {4, C});
    add("mask_decoder.output_upscaling.0.weight", {C, C / 4, 2, 2}); add("mask_decoder.output_upscaling.0.bias", {C / 4});
    add("mask_decoder.output_upscaling.1.weight", {C / 4}); add("mask_decoder.output_upscaling.1.bias", {C / 4});
    add("mask_decoder.output_upscaling.3.weight", {C / 4, C / 8, 2, 2}); add("mask_decoder.output_upscaling.3.bias", {C / 8});
    for (int i = 0; i < 4; ++i) {
        const std::string p = "mask_decoder.output_hypernetworks_mlps." + std::to_string(i) + ".layers";
        add(p + ".0.weight", {C, C}); add(p + ".0.bias", {C});
        add(p + ".1.weight", {C, C}); add(p + ".1.bias", {C});
        add(p + ".2.weight", {C / 8, C}); add(p + ".2.bias", {C / 8});
    }
    const std::string p = "mask_decoder.iou_prediction_head.layers";
    add(p + ".0.weight", {C, C}); add(p + ".0.bias", {C});
    add(p + ".1.weight", {C, C}); add(p + ".1.bias", {C});
    add(p + ".2.weight", {4, C}); add(p + ".2.bias", {4});
}

DecAttn dec_attn(samrs_engine* e, const std::string& p) {
    return DecAttn{W(e, p + ".q_proj.weight"), W(e, p + ".q_proj.bias"), W(e, p + ".k_proj.weight"),
                   W(e, p + ".k_proj.bias"),   W(e, p + ".v_proj.weight"), W(e, p + ".v_proj.bias"),
                   W(e, p + ".out_proj.weight"), W(e, p + ".out_proj.bias")};
}

DecWeights dec_weights(samrs_engine* e) {
    DecWeights d;
    d.prompt.gauss = W(e, "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix");
    for (int i = 0; i < 4; ++i) d.prompt.point_emb[i] = W(e, "prompt_encoder.point_embeddings." + std::to_string(i) + ".weight");
    d.prompt.not_a_point = W(e, "prompt_encoder.not_a_point_embed.weight");
    d.prompt.iou_token = W(e, "mask_decoder.iou_token.weight");
    d.prompt.mask_tokens = W(e, "mask_decoder.mask_tokens.weight");
    const std::string md = "prompt_encoder.mask_downscaling.";
    d.mask_embed = MaskEmbedParams{W(e, md + "0.weight"), W(e, md + "0.bias"), W(e, md + "1.weight"), W(e, md + "1.bias"),
                                   W(e, md + "3.weight"), W(e, md + "3.bias"), W(e, md + "4.weight"), W(e, md + "4.bias"),
                                   W(e, md + "6.weight"), W(e, md + "6.bias")};
    d.no_mask_embed = W(e, "prompt_encoder.no_mask_embed.weight");
    d.norm_final_w = W(e, "mask_decoder.transformer.norm_final_attn.weight");
    d.norm_final_b = W(e, "mask_decoder.transformer.norm_final_attn.bias");
    d.up_ln_w = W(e, "mask_decoder.output_upscaling.1.weight");
    d.up_ln_b = W(e, "mask_decoder.output_upscaling.1.bias");
    for (int i = 0; i < 5; ++i) {
        const std::string p = i < 4 ? "mask_decoder.output_hypernetworks_mlps." + std::to_string(i) + ".layers." : "mask_decoder.iou_prediction_head.layers.";
        for (int k = 0; k < 3; ++k) {
            d.head_w[i][k] = W(e, p + std::to_string(k) + ".weight");
            d.head_b[i][k] = W(e, p + std::to_string(k) + ".bias");
        }
    }
    return d;
}

// fp32 device tensor -> new ET device tensor (and, if asked for, the remainder of its two-term split); optionally frees the fp32 copy
int to_et(samrs_engine* e, const std::string& name, uint16_t** out, bool free_f32, hipStream_t s, uint16_t** out_lo = nullptr) {
    DevTensor& t = e->w.at(name);
    CK(e, dalloc(e, out, t.numel));
    if (out_lo) CK(e, dalloc(e, out_lo, t.numel));
    CK(e, launch_convert(e->prec, t.p, *out, (long)t.numel, s, out_lo ? *out_lo : nullptr));
    if (free_f32) {
        CK(e, hipStreamSynchronize(s));
        for (auto it = e->owned.begin(); it != e->owned.end(); ++it)
            if (*it == t.p) { e->owned.erase(it); break; }
        CK(e, hipFree(t.p));
        t.p = nullptr;
    }
    return SAMRS_OK;
}

// Outlier columns of the four block GEMMs of encoder block `i`, from the fp32 weights alone (they must still be resident: call before
// to_et frees them).  score_c = (magnitude proxy of operand column c) x || W[:, c] ||; the proxies: qkv / lin1 (A = a LayerNorm
// output): |gamma_c| + |beta_c|; lin2 (A = GELU(lin1)): || W1[c, :] || rms(gamma2) + |b1_c|; proj (A = the attention output, a
// convex combination of v rows): || Wv[c, :] || rms(gamma1) + |bv_c|.  A column is picked when its score exceeds ratio x the median
// score of its GEMM; at most 32 per GEMM (the largest), ascending.  oracle/outlier_budget.py restates the rule on the CPU and prices it.
int pick_outlier_columns(samrs_engine* e, int i, hipStream_t s) {
    const int D = e->D, H = 4 * D;
    EncBlock& b = e->blocks[i];
    const std::string p = "image_encoder.blocks." + std::to_string(i);
    if (!e->oc_scratch) CK(e, dalloc(e, &e->oc_scratch, (size_t)2 * 4 * D));
    float *dcol = e->oc_scratch, *drow = e->oc_scratch + 4 * D;
    std::vector<float> qkv_col(D), qkv_row(3 * D), l1_col(D), l1_row(H), l2_col(H), pj_col(D);
    auto norms = [&](const std::string& name, int N, int K, float* col, float* row) -> int {
        CK(e, launch_weight_norms(W(e, name), N, K, dcol, row ? drow : nullptr, s));
        CK(e, hipMemcpyAsync(col, dcol, sizeof(float) * K, hipMemcpyDeviceToHost, s));
        if (row) CK(e, hipMemcpyAsync(row, drow, sizeof(float) * N, hipMemcpyDeviceToHost, s));
        CK(e, hipStreamSynchronize(s));
        return SAMRS_OK;
    };
    int rc;
    if ((rc = norms(p + ".attn.qkv.weight", 3 * D, D, qkv_col.data(), qkv_row.data()))) return rc;
    if ((rc = norms(p + ".mlp.lin1.weight", H, D, l1_col.data(), l1_row.data()))) return rc;
    if ((rc = norms(p + ".mlp.lin2.weight", D, H, l2_col.data(), nullptr))) return rc;
    if ((rc = norms(p + ".attn.proj.weight", D, D, pj_col.data(), nullptr))) return rc;
    hipError_t copy_err = hipSuccess;
    auto host = [&](const std::string& name, size_t n) {
        std::vector<float> v(n);
        const hipError_t r = hipMemcpy(v.data(), W(e, name), sizeof(float) * n, hipMemcpyDeviceToHost);
        if (r != hipSuccess) copy_err = r;
        return v;
    };
    const std::vector<float> g1 = host(p + ".norm1.weight", D), b1 = host(p + ".norm1.bias", D), g2 = host(p + ".norm2.weight", D),
                             b2 = host(p + ".norm2.bias", D), bq = host(p + ".attn.qkv.bias", 3 * D), bl = host(p + ".mlp.lin1.bias", H);
    CK(e, copy_err);
    double r1 = 0, r2 = 0;
    for (int c = 0; c < D; ++c) { r1 += (double)g1[c] * g1[c]; r2 += (double)g2[c] * g2[c]; }
    const float rms1 = (float)std::sqrt(r1 / D), rms2 = (float)std::sqrt(r2 / D);
    std::vector<float> sc[4];
    sc[0].resize(D); sc[1].resize(D); sc[2].resize(H); sc[3].resize(D);
    for (int c = 0; c < D; ++c) {
        sc[0][c] = (std::fabs(g1[c]) + std::fabs(b1[c])) * std::sqrt(qkv_col[c]);
        sc[1][c] = (std::fabs(g2[c]) + std::fabs(b2[c])) * std::sqrt(l1_col[c]);
        sc[3][c] = (std::sqrt(qkv_row[2 * D + c]) * rms1 + std::fabs(bq[2 * D + c])) * std::sqrt(pj_col[c]);
    }
    for (int c = 0; c < H; ++c) sc[2][c] = (std::sqrt(l1_row[c]) * rms2 + std::fabs(bl[c])) * std::sqrt(l2_col[c]);
    const float ratio = e->outlier_ratio_pct * 0.01f;
    for (int g = 0; g < 4; ++g) {
        std::vector<float> tmp(sc[g]);
        std::nth_element(tmp.begin(), tmp.begin() + tmp.size() / 2, tmp.end());
        const float med = tmp[tmp.size() / 2];
        std::vector<int> idx;
        for (int c = 0; c < (int)sc[g].size(); ++c) if (sc[g][c] > ratio * med) idx.push_back(c);
        if (idx.size() > 32) {
            std::partial_sort(idx.begin(), idx.begin() + 32, idx.end(), [&](int a, int c) { return sc[g][a] > sc[g][c]; });
            idx.resize(32);
            std::sort(idx.begin(), idx.end());
        }
        b.oc_n[g] = (int)idx.size();
        e->outlier_columns += b.oc_n[g];
        if (g == 3) {
            b.oc_heads = 0;
            for (int c : idx) b.oc_heads |= (e->hd > 0 && c / e->hd < 32) ? (1u << (c / e->hd)) : 0xffffffffu;
        }
        double all2 = 0.0, sel2 = 0.0;
        for (float v : sc[g]) all2 += (double)v * v;
        for (int c : idx) sel2 += (double)sc[g][c] * sc[g][c];
        b.oc_share[g] = all2 > 0.0 ? (float)(sel2 / all2) : 0.f;
        if (b.oc_n[g]) {
            CK(e, dalloc(e, &b.oc_idx[g], 32));
            idx.resize(32, 0);
            CK(e, hipMemcpy(b.oc_idx[g], idx.data(), sizeof(int) * 32, hipMemcpyHostToDevice));
        }
    }
    if (b.oc_n[0] || b.oc_n[1]) e->outlier_blocks += 1;
    if (b.oc_share[0] > 0.5f || b.oc_share[3] > 0.5f) e->outlier_dominant_blocks += 1;
    return SAMRS_OK;
}

}  // namespace

namespace samrs_detail {
hipError_t scratch_reserve(DeviceScratch& sc, size_t need, hipStream_t s) {
    if (need <= sc.bytes) return hipSuccess;
    if (sc.p) {
        hipError_t r = hipStreamSynchronize(s);
        if (r == hipSuccess) r = hipFree(sc.p);           // device-synchronising: nothing still reads the old scratch
        if (r != hipSuccess) return r;
        sc = DeviceScratch{};
    }
    const hipError_t r = hipMalloc(&sc.p, need);
    if (r == hipSuccess) sc.bytes = need; else sc.p = nullptr;
    return r;
}

void scratch_release(DeviceScratch& sc) {
    if (sc.p) (void)hipFree(sc.p);
    sc = DeviceScratch{};
}
}  // namespace samrs_detail

// =================================================================================================
extern "C" {

int samrs_abi_version(void) { return SAMRS_ABI_VERSION; }

const char* samrs_last_error(const samrs_engine_t* e) { return e ? e->err.c_str() : "null engine"; }

samrs_engine_t* samrs_create(const samrs_config* cfg, int device, char* err, int err_len) {
    auto bad = [&](const char* m) -> samrs_engine_t* {
        if (err && err_len > 0) snprintf(err, err_len, "%s", m);
        return nullptr;
    };
    if (!cfg) return bad("null config");
    if (cfg->img_size != 1024 || cfg->patch_size != 16 || cfg->window_size != 14 || cfg->out_chans != 256)
        return bad("only img_size 1024 / patch 16 / window 14 / out_chans 256 are supported (build_sam.py:62-80)");
    // What the decoder relies on from here on: grid 64, tokens 4096 in every engine that exists.  Its route (decode_route) therefore asks no
    // shape question: 32-row key groups (i2t_fused), 16-token upscaler groups, 256-row GEMM tiles and 1024-row ConvT #2 blocks all divide
    // these sizes, and each launcher refuses a shape it cannot take on its own.
    if (cfg->embed_dim % 128 || cfg->embed_dim % cfg->num_heads) return bad("embed_dim must be a multiple of 128 and of num_heads");
    const int hd = cfg->embed_dim / cfg->num_heads;
    if (hd != 64 && hd != 80) return bad("head_dim must be 64 or 80");
    if (cfg->precision != SAMRS_PREC_BF16 && cfg->precision != SAMRS_PREC_F16) return bad("bad precision");
    if (cfg->max_images < 1 || cfg->max_prompts < 1 || cfg->max_points < 0 || cfg->n_global < 0 || cfg->n_global > 8)
        return bad("bad capacity / n_global");
    if (5 + cfg->max_points + 1 + 2 > 16) return bad("max_points too large (token count must stay <= 16)");
    {
        DeviceGuard dg(device);
        if (dg.status != hipSuccess) return bad("hipSetDevice failed (no HIP device? this library has no CPU fallback)");
    }
    samrs_engine* e = new samrs_engine();
    e->cfg = *cfg;
    e->device = device;
    e->prec = cfg->precision;
    e->grid = cfg->img_size / cfg->patch_size;
    e->tokens = e->grid * e->grid;
    e->D = cfg->embed_dim;
    e->C = cfg->out_chans;
    e->hd = hd;
    e->nwin = (e->grid + cfg->window_size - 1) / cfg->window_size;
    e->T_max = 5 + cfg->max_points + 1 + 2;
    e->decode_prompts = cfg->max_prompts;
    e->slot_set.assign(cfg->max_images, 0);
    e->slot_split.assign(cfg->max_images, 0);
    e->slot_depth.assign(cfg->max_images, 0);
    e->decoder_fusion = env_int("SAMRS_DECODER_FUSION", 1) != 0;
    e->ln_fold = env_int("SAMRS_LN_FOLD", 0) != 0 && gemm_has_experiments();
    // default: the cheap rounding points everywhere; where the one-launch split GEMM covers the block shapes (ViT-H), also the
    // v third of qkv + proj in the leading blocks -- that is what it takes to hold IoU >= 0.999 on the multimask (C4)
    // fixtures at ViT-H, for 0.90x the throughput.  SAMRS_SPLIT=15 / option "split" = 15: the 1x-rate arithmetic.
    const bool h_like = gemm_split3_ok(e->tokens, 3 * e->D, e->D) && gemm_split3_ok(e->tokens, e->D, e->D) && (2 * e->D) % 320 == 0;
    e->split = env_int("SAMRS_SPLIT", SPLIT_DEFAULT | (h_like ? SPLIT_ATTN_V : 0)) & SPLIT_ALL;
    // ViT-H: the multimask tokens hold IoU >= 0.999 only from the v-third / proj split on; below ViT-H the 1x rate does
    e->grade_multimask = h_like ? SPLIT_ATTN_ANY : 0;
    // an explicit SAMRS_SPLIT is the operator's decision about the whole process, multimask outputs included
    e->allow_reduced = env_int("SAMRS_ALLOW_REDUCED", getenv("SAMRS_SPLIT") ? 1 : 0) != 0;
    e->upscaler_fused = env_int("SAMRS_UPSCALER_FUSED", 1) != 0;
    e->split_passes = env_int("SAMRS_SPLIT_PASSES", 0) != 0;
    e->split_depth = env_int("SAMRS_SPLIT_DEPTH", 0);
    e->lo_format = (h_like && env_int("SAMRS_LO_FORMAT", 4) == 4) ? 4 : 0;
    e->gelu_fast = env_int("SAMRS_GELU_FAST", -1);
    e->ln_tail = env_int("SAMRS_LN_TAIL", 0) != 0;
    e->operand_pad_on = env_int("SAMRS_OPERAND_PAD", 1) != 0;
    e->outlier_on = env_int("SAMRS_OUTLIER_COLS", 7) & 7;
    e->outlier_ratio_pct = env_int("SAMRS_OUTLIER_RATIO_PCT", 400);
    if (e->outlier_ratio_pct < 101) e->outlier_ratio_pct = 101;
    if (e->gelu_fast > 1) e->gelu_fast = 1;
    e->range_profile = env_int("SAMRS_RANGE_PROFILE", 0);
    if (e->range_profile < 0 || e->range_profile > 2) e->range_profile = 0;
    e->audit_passes = env_int("SAMRS_AUDIT_PASSES", 0);
    if (e->audit_passes > 0) e->range_profile = 2; else e->audit_passes = 0;
    if (const int rc0 = env_int("SAMRS_RANGE_CHECK", 0)) {
        if (samrs_set_option(e, "range_check", rc0) != SAMRS_OK) {
            if (err && err_len > 0) snprintf(err, err_len, "SAMRS_RANGE_CHECK=%d: %s", rc0, e->err.c_str());
            samrs_destroy(e);
            return nullptr;
        }
    }
    return e;
}

void samrs_destroy(samrs_engine_t* e) {
    if (!e) return;
    DeviceGuard dg(e->device);
    for (void* p : e->owned) (void)hipFree(p);
    for (DeviceScratch* sc : {&e->rle_scratch, &e->rle_decode_scratch, &e->region_scratch, &e->box_scratch, &e->poly_scratch, &e->png_scratch, &e->png_rgb_scratch, &e->overlap_scratch, &e->ap_scratch, &e->boundary_scratch}) scratch_release(*sc);
    delete e;
}

int samrs_load_weight(samrs_engine_t* e, const char* name, const float* host, const int64_t* shape, int ndim) {
    if (!e || !name || !host || !shape || ndim < 1 || ndim > 4) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_load_weight: bad argument");
    if (e->finalized) return fail(e, SAMRS_ERR_BAD_WEIGHTS, "weights already finalized");
    ON_DEVICE(e);
    DevTensor t;
    t.shape.assign(shape, shape + ndim);
    t.numel = 1;
    for (int i = 0; i < ndim; ++i) t.numel *= (size_t)shape[i];
    const std::string n(name);
    std::vector<float> tmp;
    const float* src = host;
    if (n == "image_encoder.neck.2.weight" && ndim == 4) {
        // [co][ci][ky][kx] -> [co][(ky*3+kx)*Ci + ci]  (k order of neck_im2col_kernel)
        const int64_t Co = shape[0], Ci = shape[1], KH = shape[2], KW = shape[3];
        tmp.resize(t.numel);
        for (int64_t co = 0; co < Co; ++co)
            for (int64_t ci = 0; ci < Ci; ++ci)
                for (int64_t ky = 0; ky < KH; ++ky)
                    for (int64_t kx = 0; kx < KW; ++kx)
                        tmp[(co * KH * KW + ky * KW + kx) * Ci + ci] = host[((co * Ci + ci) * KH + ky) * KW + kx];
        src = tmp.data();
    } else if ((n == "mask_decoder.output_upscaling.0.weight" || n == "mask_decoder.output_upscaling.3.weight") && ndim == 4) {
        // ConvTranspose2d [ci][co][dy][dx] -> GEMM B [(dy*2+dx)*Co + co][ci]   (mask_decoder.py:53-59)
        const int64_t Ci = shape[0], Co = shape[1];
        tmp.resize(t.numel);
        for (int64_t ci = 0; ci < Ci; ++ci)
            for (int64_t co = 0; co < Co; ++co)
                for (int64_t s = 0; s < 4; ++s) tmp[(s * Co + co) * Ci + ci] = host[(ci * Co + co) * 4 + s];
        src = tmp.data();
    }
    auto it = e->w.find(n);
    if (it != e->w.end()) return fail(e, SAMRS_ERR_BAD_WEIGHTS, "duplicate tensor %s", name);
    CK(e, dalloc(e, &t.p, t.numel));
    CK(e, hipMemcpy(t.p, src, t.numel * sizeof(float), hipMemcpyHostToDevice));
    e->w.emplace(n, std::move(t));
    return SAMRS_OK;
}
}  // extern "C"

// ---- the per-prompt decoder workspaces ------------------------------------------------------------------------------------------------
// Every buffer of the decoder pass whose size is a number of prompts, with its bytes per prompt, listed ONCE: samrs_finalize_weights
// (capacity = max_prompts unless option "decode_prompts" was set before it) and a later growth of "decode_prompts" both go through
// grow_decode_workspaces, so the two cannot drift apart.  `lazy`: allocated by the first pass that needs the buffer (need_decode_buffer),
// at the capacity of that moment, and grown with the others from then on.
// The largest element index on the pass is KVQ's n x 4096 x 384 (U2: n x 2^21), the largest byte offset n x 2^22 (KF, U1raw, U2):
// up to DECODE_PROMPTS_LIMIT prompts every index AND byte offset of a chain stays below 2^31, whatever type a kernel counts in;
// every launcher's blockIdx.y = n stays far below 65536.
constexpr int DECODE_PROMPTS_LIMIT = 512;

struct DecodeBuf {
    const char* name;
    size_t per_prompt;             // bytes
    bool lazy;
    void* (*get)(const samrs_engine_t*);
    void (*set)(samrs_engine_t*, void*);
};
#define DECODE_BUF(field, elems, lazy)                                                             \
    DecodeBuf{#field, sizeof(*static_cast<samrs_engine_t*>(nullptr)->field) * (size_t)(elems), lazy, \
              [](const samrs_engine_t* e) -> void* { return e->field; },                           \
              [](samrs_engine_t* e, void* p) { e->field = static_cast<decltype(e->field)>(p); }}

static std::vector<DecodeBuf> decode_buffers(const samrs_engine_t* e) {
    const size_t T = (size_t)e->T_max, tokens = (size_t)e->tokens, C = (size_t)e->C, Ci = C / 2;
    return {
        // token side: [Bb * T_max] rows
        DECODE_BUF(TOK0, T * C, false), DECODE_BUF(Q, T * C, false), DECODE_BUF(TA, T * C, false), DECODE_BUF(TQ, T * C, false),
        DECODE_BUF(TK, T * C, false), DECODE_BUF(TV, T * C, false), DECODE_BUF(TO, T * C, false), DECODE_BUF(MH, T * 2048, false),
        DECODE_BUF(QP, T * Ci, false), DECODE_BUF(KT, T * Ci, false), DECODE_BUF(VT, T * Ci, false), DECODE_BUF(O128, T * Ci, false),
        DECODE_BUF(T2IW, t2i_workspace_floats(1, e->T_max), false),        // linear in the prompt count (T2I_MAX_SPLITS partial states each)
        // image side: [Bb * tokens] rows
        DECODE_BUF(KF, tokens * C, false), DECODE_BUF(KE, tokens * C, false), DECODE_BUF(KE_lo, tokens * C, false),
        DECODE_BUF(KVQ, tokens * 3 * Ci, false), DECODE_BUF(OI, tokens * Ci, false),
        DECODE_BUF(DENSE, tokens * C, true), DECODE_BUF(SLOT_OF, 1, true),
        DECODE_BUF(U1raw, tokens * C, true), DECODE_BUF(U1, tokens * C, true), DECODE_BUF(U2, tokens * 4 * Ci, true),
        // heads and outputs
        DECODE_BUF(HY1, 5 * C, false), DECODE_BUF(HY2, 5 * C, false), DECODE_BUF(HYPER, 4 * (C / 8), false), DECODE_BUF(IOU, 4, false),
        DECODE_BUF(LOW, 3 * 256 * 256, false),
    };
}
#undef DECODE_BUF

// The buffers hold at least `cap` prompts afterwards.  Contents are not carried over: everything listed is scratch of one chain.  No
// chain may be running on another host thread (an engine is driven by one thread at a time).  Old buffers are released only after
// every stream of the device has drained -- the chains that used them may have run on any -- and a failed allocation leaves the
// engine as it was.  Never shrinks.
static int grow_decode_workspaces(samrs_engine_t* e, int cap) {
    if (cap <= e->decode_alloc) return SAMRS_OK;
    const std::vector<DecodeBuf> bufs = decode_buffers(e);
    std::vector<void*> fresh(bufs.size(), nullptr);
    size_t bytes = 0;
    for (size_t i = 0; i < bufs.size(); ++i) {
        if (bufs[i].lazy && !bufs[i].get(e)) continue;
        const hipError_t r = hipMalloc(&fresh[i], bufs[i].per_prompt * (size_t)cap);
        if (r != hipSuccess) {
            for (void* p : fresh) if (p) (void)hipFree(p);
            return fail(e, SAMRS_ERR_HIP, "decoder workspaces for %d prompts: %s (%zu bytes for %s)", cap, hipGetErrorString(r),
                        bufs[i].per_prompt * (size_t)cap, bufs[i].name);
        }
        bytes += bufs[i].per_prompt * (size_t)cap;
    }
    if (e->decode_alloc > 0) CK(e, hipDeviceSynchronize());
    for (size_t i = 0; i < bufs.size(); ++i) {
        if (!fresh[i]) continue;
        if (void* old = bufs[i].get(e)) {
            e->owned.erase(std::find(e->owned.begin(), e->owned.end(), old));
            (void)hipFree(old);
        }
        e->owned.push_back(fresh[i]);
        bufs[i].set(e, fresh[i]);
    }
    e->decode_alloc = cap;
    e->decode_bytes = bytes;
    return SAMRS_OK;
}

namespace samrs_detail {
// a lazy buffer of the list, by its field name, at the current capacity
int need_decode_buffer(samrs_engine_t* e, const char* name) {
    for (const DecodeBuf& b : decode_buffers(e)) {
        if (strcmp(b.name, name)) continue;
        if (b.get(e)) return SAMRS_OK;
        void* p = nullptr;
        CK(e, hipMalloc(&p, b.per_prompt * (size_t)e->decode_alloc));
        e->owned.push_back(p);
        b.set(e, p);
        e->decode_bytes += b.per_prompt * (size_t)e->decode_alloc;
        return SAMRS_OK;
    }
    return fail(e, SAMRS_ERR_BAD_ARG, "no decoder workspace named %s", name);
}
}  // namespace samrs_detail

extern "C" {
int samrs_finalize_weights(samrs_engine_t* e, void* stream) {
    if (!e) return SAMRS_ERR_BAD_ARG;
    if (e->finalized) return SAMRS_OK;
    hipStream_t s = (hipStream_t)stream;
    ON_DEVICE(e);
    // ---- strict check (build_sam.py:106 load_state_dict raises on any mismatch) ----
    std::vector<std::pair<std::string, std::vector<int64_t>>> req;
    required_tensors(e, req);
    for (auto& r : req) {
        auto it = e->w.find(r.first);
        if (it == e->w.end()) return fail(e, SAMRS_ERR_BAD_WEIGHTS, "missing tensor %s", r.first.c_str());
        if (it->second.shape != r.second) return fail(e, SAMRS_ERR_BAD_WEIGHTS, "shape mismatch for %s", r.first.c_str());
    }
    if (e->w.size() != req.size()) {
        for (auto& kv : e->w) {
            bool found = false;
            for (auto& r : req) if (r.first == kv.first) { found = true; break; }
            if (!found) return fail(e, SAMRS_ERR_BAD_WEIGHTS, "unexpected tensor %s", kv.first.c_str());
        }
    }
    const samrs_config& c = e->cfg;
    const int D = e->D, C = e->C, tokens = e->tokens;
    int rc;
    // ---- encoder weights -> ET ----
    if ((rc = to_et(e, "image_encoder.patch_embed.proj.weight", &e->patch_w, true, s, &e->patch_w_lo))) return rc;
    if ((rc = to_et(e, "image_encoder.neck.0.weight", &e->neck0_w, true, s, &e->neck0_w_lo))) return rc;
    if ((rc = to_et(e, "image_encoder.neck.2.weight", &e->neck2_w, true, s, &e->neck2_w_lo))) return rc;
    e->blocks.resize(c.depth);
    for (int i = 0; i < c.depth; ++i) {
        const std::string p = "image_encoder.blocks." + std::to_string(i);
        EncBlock& b = e->blocks[i];
        b.global = is_global(c, i);
        // padded operand rows (field ldk) exist where a D-element row is an even number of 256-byte units AND the qkv / lin1 shapes can
        // run on the kernels that take a stride (N a multiple of 320): ViT-H
        if (i == 0) e->ldk = (e->operand_pad_on && D % 256 == 0 && (3 * D) % 320 == 0 && (4 * D) % 320 == 0) ? D + 128 : 0;
        b.ln1w = W(e, p + ".norm1.weight"); b.ln1b = W(e, p + ".norm1.bias");
        b.ln2w = W(e, p + ".norm2.weight"); b.ln2b = W(e, p + ".norm2.bias");
        if (D == 1280 && e->ln_fold && gemm_has_experiments()) {       // folded LayerNorm needs the fp32 weights: before to_et() frees them
            CK(e, dalloc(e, &b.qkv_wf, (size_t)3 * D * D)); CK(e, dalloc(e, &b.qkv_c, (size_t)3 * D)); CK(e, dalloc(e, &b.qkv_bf, (size_t)3 * D));
            CK(e, dalloc(e, &b.lin1_wf, (size_t)4 * D * D)); CK(e, dalloc(e, &b.lin1_c, (size_t)4 * D)); CK(e, dalloc(e, &b.lin1_bf, (size_t)4 * D));
            CK(e, launch_ln_fold_weight(e->prec, W(e, p + ".attn.qkv.weight"), b.ln1w, b.ln1b, W(e, p + ".attn.qkv.bias"), b.qkv_wf,
                                        b.qkv_c, b.qkv_bf, 3 * D, D, s));
            CK(e, launch_ln_fold_weight(e->prec, W(e, p + ".mlp.lin1.weight"), b.ln2w, b.ln2b, W(e, p + ".mlp.lin1.bias"), b.lin1_wf,
                                        b.lin1_c, b.lin1_bf, 4 * D, D, s));
            e->can_fold = true;
        }
        const bool lo_a = (e->split & SPLIT_ATTN_ANY) != 0, lo_m = (e->split & SPLIT_MLP) != 0, lo_l2 = (e->split & SPLIT_LIN2) != 0;
        if (lo_a && e->lo_format == 4 && gemm_mx_ok(c.max_images * e->tokens, 3 * D, D, D)) {
            // fp4 copies of hi / lo of the attention-side weights (from the fp32 tensors, before to_et frees them)
            const int gp = (e->hd + 31) / 32 * 32, kp = c.num_heads * gp;
            if (gemm_mx_ok(c.max_images * e->tokens, D, D, kp)) {
                e->mx_gp = gp; e->mx_kp_proj = kp;
                for (int h = 0; h < 2; ++h) {
                    CK(e, dalloc(e, &b.qkv_w4[h], (size_t)3 * D * D / 2)); CK(e, dalloc(e, &b.qkv_s4[h], mx_scale_bytes(3 * D, D, true)));
                    CK(e, dalloc(e, &b.proj_w4[h], (size_t)D * kp / 2)); CK(e, dalloc(e, &b.proj_s4[h], mx_scale_bytes(D, kp, true)));
                }
                CK(e, launch_mx4_pack(e->prec, W(e, p + ".attn.qkv.weight"), nullptr, nullptr, nullptr, b.qkv_w4[0], b.qkv_w4[1], b.qkv_s4[0],
                                      b.qkv_s4[1], 3 * D, D, D, D, true, s));
                CK(e, launch_mx4_pack(e->prec, W(e, p + ".attn.proj.weight"), nullptr, nullptr, nullptr, b.proj_w4[0], b.proj_w4[1], b.proj_s4[0],
                                      b.proj_s4[1], D, D, e->hd, gp, true, s, /* perm: the attention kernels' block order */ true));
                e->mx_ready = true;
            }
        }
        if ((lo_m || lo_l2) && e->lo_format == 4 && gemm_mx_ok(c.max_images * e->tokens, 4 * D, D, D) && (4 * D) % 80 == 0) {
            const int kp2 = 4 * D / 80 * 96;
            if (gemm_mx_ok(c.max_images * e->tokens, D, 4 * D, kp2)) {
                e->mx_kp_lin2 = kp2;
                for (int h = 0; h < 2; ++h) {
                    CK(e, dalloc(e, &b.lin1_w4[h], (size_t)4 * D * D / 2)); CK(e, dalloc(e, &b.lin1_s4[h], mx_scale_bytes(4 * D, D, true)));
                    CK(e, dalloc(e, &b.lin2_w4[h], (size_t)D * kp2 / 2)); CK(e, dalloc(e, &b.lin2_s4[h], mx_scale_bytes(D, kp2, true)));
                }
                CK(e, launch_mx4_pack(e->prec, W(e, p + ".mlp.lin1.weight"), nullptr, nullptr, nullptr, b.lin1_w4[0], b.lin1_w4[1], b.lin1_s4[0],
                                      b.lin1_s4[1], 4 * D, D, D, D, true, s));
                CK(e, launch_mx4_pack(e->prec, W(e, p + ".mlp.lin2.weight"), nullptr, nullptr, nullptr, b.lin2_w4[0], b.lin2_w4[1], b.lin2_s4[0],
                                      b.lin2_s4[1], D, 4 * D, 80, 96, true, s, /* perm: the order of lin1's epilogue */ 2));
                e->mx_mlp_ready = true;
            }
        }
        // outlier columns: picked and their weight-side extension written while the fp32 weights are still resident
        if (e->outlier_on && (rc = pick_outlier_columns(e, i, s))) return rc;
        if (e->ldk) {
            const size_t ldb = (size_t)e->ldk * 2;
            CK(e, dalloc(e, &b.qkv_wp, (size_t)3 * D * e->ldk)); CK(e, dalloc(e, &b.lin1_wp, (size_t)4 * D * e->ldk));
            CK(e, hipMemsetAsync(b.qkv_wp, 0, (size_t)3 * D * ldb, s)); CK(e, hipMemsetAsync(b.lin1_wp, 0, (size_t)4 * D * ldb, s));
            if (b.oc_n[0]) CK(e, launch_outlier_weight_ext(e->prec, W(e, p + ".attn.qkv.weight"), 3 * D, D, b.oc_idx[0], b.oc_n[0], b.qkv_wp, e->ldk, D, s));
            if (b.oc_n[1]) CK(e, launch_outlier_weight_ext(e->prec, W(e, p + ".mlp.lin1.weight"), 4 * D, D, b.oc_idx[1], b.oc_n[1], b.lin1_wp, e->ldk, D, s));
        }
        if (b.oc_n[0]) {
            CK(e, dalloc(e, &b.qkv_wx, (size_t)3 * D * (D + 64)));
            CK(e, launch_outlier_weight_ext(e->prec, W(e, p + ".attn.qkv.weight"), 3 * D, D, b.oc_idx[0], b.oc_n[0], b.qkv_wx, D + 64, D, s));
        }
        if (b.oc_n[1]) {
            CK(e, dalloc(e, &b.lin1_wx, (size_t)4 * D * (D + 64)));
            CK(e, launch_outlier_weight_ext(e->prec, W(e, p + ".mlp.lin1.weight"), 4 * D, D, b.oc_idx[1], b.oc_n[1], b.lin1_wx, D + 64, D, s));
        }
        if (b.oc_n[2]) {          // lin2: weight side [D][64] + the side weights / bias of the hidden units' recomputation
            CK(e, dalloc(e, &b.oc_bx[2], (size_t)D * 64));
            CK(e, launch_outlier_weight_ext(e->prec, W(e, p + ".mlp.lin2.weight"), D, 4 * D, b.oc_idx[2], b.oc_n[2], b.oc_bx[2], 64, 0, s));
            CK(e, dalloc(e, &b.lin2_sb, (size_t)32));
            const int k0 = D + (b.oc_n[1] ? 64 : 0);
            CK(e, dalloc(e, &b.lin2_ws, (size_t)32 * k0));
            CK(e, launch_outlier_side_weight(e->prec, W(e, p + ".mlp.lin1.weight"), W(e, p + ".mlp.lin1.bias"), D, b.oc_idx[2], b.oc_n[2],
                                             b.oc_idx[1], b.oc_n[1], b.lin2_ws, k0, b.lin2_sb, s));
            e->oc_resid = true;
        }
        if (b.oc_n[3]) {          // proj
            CK(e, dalloc(e, &b.oc_bx[3], (size_t)D * 64));
            CK(e, launch_outlier_weight_ext(e->prec, W(e, p + ".attn.proj.weight"), D, D, b.oc_idx[3], b.oc_n[3], b.oc_bx[3], 64, 0, s));
            e->oc_resid = true;
        }
        if ((rc = to_et(e, p + ".attn.qkv.weight", &b.qkv_w, true, s, lo_a ? &b.qkv_w_lo : nullptr))) return rc;
        if ((rc = to_et(e, p + ".attn.proj.weight", &b.proj_w, true, s, lo_a ? &b.proj_w_lo : nullptr))) return rc;
        if ((rc = to_et(e, p + ".mlp.lin1.weight", &b.lin1_w, true, s, lo_m ? &b.lin1_w_lo : nullptr))) return rc;
        if ((rc = to_et(e, p + ".mlp.lin2.weight", &b.lin2_w, true, s, lo_m ? &b.lin2_w_lo : nullptr))) return rc;
        {
            const size_t wb = (size_t)D * 2;
            if (e->ldk) {
                const size_t ldb = (size_t)e->ldk * 2;
                CK(e, hipMemcpy2DAsync(b.qkv_wp, ldb, b.qkv_w, wb, wb, (size_t)3 * D, hipMemcpyDeviceToDevice, s));
                CK(e, hipMemcpy2DAsync(b.lin1_wp, ldb, b.lin1_w, wb, wb, (size_t)4 * D, hipMemcpyDeviceToDevice, s));
            }
            const size_t ldx = (size_t)(D + 64) * 2;
            if (b.qkv_wx) CK(e, hipMemcpy2DAsync(b.qkv_wx, ldx, b.qkv_w, wb, wb, (size_t)3 * D, hipMemcpyDeviceToDevice, s));
            if (b.lin1_wx) CK(e, hipMemcpy2DAsync(b.lin1_wx, ldx, b.lin1_w, wb, wb, (size_t)4 * D, hipMemcpyDeviceToDevice, s));
        }
        b.ln1w = W(e, p + ".norm1.weight"); b.ln1b = W(e, p + ".norm1.bias");
        b.ln2w = W(e, p + ".norm2.weight"); b.ln2b = W(e, p + ".norm2.bias");
        b.qkv_b = W(e, p + ".attn.qkv.bias"); b.proj_b = W(e, p + ".attn.proj.bias");
        b.lin1_b = W(e, p + ".mlp.lin1.bias"); b.lin2_b = W(e, p + ".mlp.lin2.bias");
        b.rel_h = W(e, p + ".attn.rel_pos_h"); b.rel_w = W(e, p + ".attn.rel_pos_w");
    }
    // ---- decoder: dense PE, fused image-side projection weights, PE projections ----
    CK(e, dalloc(e, &e->PE, (size_t)tokens * C));
    CK(e, launch_dense_pe(W(e, "prompt_encoder.pe_layer.positional_encoding_gaussian_matrix"), e->PE, e->grid, s));
    const int Ci = C / 2;  // 128
    float* tmpw = nullptr;
    CK(e, dalloc(e, &tmpw, (size_t)3 * Ci * C));
    e->layers.resize(2);
    for (int i = 0; i < 2; ++i) {
        const std::string p = "mask_decoder.transformer.layers." + std::to_string(i);
        DecLayer& L = e->layers[i];
        L.self = dec_attn(e, p + ".self_attn");
        L.t2i = dec_attn(e, p + ".cross_attn_token_to_image");
        L.i2t = dec_attn(e, p + ".cross_attn_image_to_token");
        L.n1w = W(e, p + ".norm1.weight"); L.n1b = W(e, p + ".norm1.bias");
        L.n2w = W(e, p + ".norm2.weight"); L.n2b = W(e, p + ".norm2.bias");
        L.n3w = W(e, p + ".norm3.weight"); L.n3b = W(e, p + ".norm3.bias");
        L.n4w = W(e, p + ".norm4.weight"); L.n4b = W(e, p + ".norm4.bias");
        L.m1w = W(e, p + ".mlp.lin1.weight"); L.m1b = W(e, p + ".mlp.lin1.bias");
        L.m2w = W(e, p + ".mlp.lin2.weight"); L.m2b = W(e, p + ".mlp.lin2.bias");
        // [Wk_t2i; Wv_t2i; Wq_i2t]
        CK(e, hipMemcpyAsync(tmpw, L.t2i.kw, sizeof(float) * Ci * C, hipMemcpyDeviceToDevice, s));
        CK(e, hipMemcpyAsync(tmpw + Ci * C, L.t2i.vw, sizeof(float) * Ci * C, hipMemcpyDeviceToDevice, s));
        CK(e, hipMemcpyAsync(tmpw + 2 * Ci * C, L.i2t.qw, sizeof(float) * Ci * C, hipMemcpyDeviceToDevice, s));
        CK(e, dalloc(e, &L.kvq_w, (size_t)3 * Ci * C));
        CK(e, launch_convert(e->prec, tmpw, L.kvq_w, (long)3 * Ci * C, s));
        CK(e, dalloc(e, &L.kvq_b, (size_t)3 * Ci));
        CK(e, hipMemcpyAsync(L.kvq_b, L.t2i.kb, sizeof(float) * Ci, hipMemcpyDeviceToDevice, s));
        CK(e, hipMemcpyAsync(L.kvq_b + Ci, L.t2i.vb, sizeof(float) * Ci, hipMemcpyDeviceToDevice, s));
        CK(e, hipMemcpyAsync(L.kvq_b + 2 * Ci, L.i2t.qb, sizeof(float) * Ci, hipMemcpyDeviceToDevice, s));
        CK(e, dalloc(e, &L.kvq_pe, (size_t)tokens * 3 * Ci));
        CK(e, hipMemsetAsync(L.kvq_pe, 0, sizeof(float) * tokens * 3 * Ci, s));
        CK(e, launch_gemm_f32(e->PE, C, L.t2i.kw, nullptr, L.kvq_pe, 3 * Ci, tokens, Ci, C, false, false, s));
        CK(e, launch_gemm_f32(e->PE, C, L.i2t.qw, nullptr, L.kvq_pe + 2 * Ci, 3 * Ci, tokens, Ci, C, false, false, s));
        if ((rc = to_et(e, p + ".cross_attn_image_to_token.out_proj.weight", &L.i2t_ow, false, s, &L.i2t_ow_lo))) return rc;
    }
    e->fin = dec_attn(e, "mask_decoder.transformer.final_attn_token_to_image");
    CK(e, hipMemcpyAsync(tmpw, e->fin.kw, sizeof(float) * Ci * C, hipMemcpyDeviceToDevice, s));
    CK(e, hipMemcpyAsync(tmpw + Ci * C, e->fin.vw, sizeof(float) * Ci * C, hipMemcpyDeviceToDevice, s));
    CK(e, dalloc(e, &e->fin_kv_w, (size_t)2 * Ci * C));
    CK(e, launch_convert(e->prec, tmpw, e->fin_kv_w, (long)2 * Ci * C, s));
    CK(e, dalloc(e, &e->fin_kv_b, (size_t)2 * Ci));
    CK(e, hipMemcpyAsync(e->fin_kv_b, e->fin.kb, sizeof(float) * Ci, hipMemcpyDeviceToDevice, s));
    CK(e, hipMemcpyAsync(e->fin_kv_b + Ci, e->fin.vb, sizeof(float) * Ci, hipMemcpyDeviceToDevice, s));
    CK(e, dalloc(e, &e->fin_pe, (size_t)tokens * 2 * Ci));
    CK(e, hipMemsetAsync(e->fin_pe, 0, sizeof(float) * tokens * 2 * Ci, s));
    CK(e, launch_gemm_f32(e->PE, C, e->fin.kw, nullptr, e->fin_pe, 2 * Ci, tokens, Ci, C, false, false, s));
    // upscaler: weights were reordered at load to GEMM-B layout; biases are tiled over the 4 sub-pixels
    if ((rc = to_et(e, "mask_decoder.output_upscaling.0.weight", &e->up1_w, false, s, &e->up1_w_lo))) return rc;
    if ((rc = to_et(e, "mask_decoder.output_upscaling.3.weight", &e->up2_w, false, s, &e->up2_w_lo))) return rc;
    CK(e, dalloc(e, &e->up1_b, (size_t)C));
    CK(e, dalloc(e, &e->up2_b, (size_t)C / 2));
    CK(e, dalloc(e, &e->up_ln, (size_t)C / 2));
    CK(e, hipMemcpyAsync(e->up_ln, W(e, "mask_decoder.output_upscaling.1.weight"), sizeof(float) * C / 4, hipMemcpyDeviceToDevice, s));
    CK(e, hipMemcpyAsync(e->up_ln + C / 4, W(e, "mask_decoder.output_upscaling.1.bias"), sizeof(float) * C / 4, hipMemcpyDeviceToDevice, s));
    for (int k = 0; k < 4; ++k) {
        CK(e, hipMemcpyAsync(e->up1_b + k * (C / 4), W(e, "mask_decoder.output_upscaling.0.bias"), sizeof(float) * C / 4, hipMemcpyDeviceToDevice, s));
        CK(e, hipMemcpyAsync(e->up2_b + k * (C / 8), W(e, "mask_decoder.output_upscaling.3.bias"), sizeof(float) * C / 8, hipMemcpyDeviceToDevice, s));
    }

    // ---- workspaces ----
    const size_t Bi = c.max_images;
    const size_t M = Bi * tokens;
    const size_t Mmax = M;
    CK(e, dalloc(e, &e->X, M * D));
    CK(e, dalloc(e, &e->ln_counters, M / 256 + 1));
    CK(e, hipMemsetAsync(e->ln_counters, 0, (M / 256 + 1) * sizeof(unsigned int), s));
    const size_t y_ld_max = e->ldk ? (size_t)e->ldk : (e->outlier_blocks ? (size_t)D + 64 : (size_t)D);    // ldk = D + 128 holds the 64 extension columns too
    CK(e, dalloc(e, &e->Y, Mmax * y_ld_max));
    CK(e, hipMemsetAsync(e->Y, 0, Mmax * y_ld_max * 2, s));
    if (e->can_fold) { CK(e, dalloc(e, &e->STATS, Mmax * 16)); CK(e, dalloc(e, &e->ROWSTAT, Mmax * 2)); }
    CK(e, dalloc(e, &e->QKV, Mmax * 3 * D));
    CK(e, dalloc(e, &e->AO, M * D));
    CK(e, dalloc(e, &e->VTG, M * D));
    if (e->oc_resid) {
        CK(e, dalloc(e, &e->OCX, M * 64));
        if (!(e->split & SPLIT_ATTN_ANY)) CK(e, dalloc(e, &e->AOlo, M * D));       // proj's outlier columns take the attention output's lo half
    }
    e->split_ready = SPLIT_DEFAULT | (e->split & SPLIT_MLP) | ((e->split & SPLIT_ATTN_ANY) ? SPLIT_ATTN_ANY : 0) | (e->mx_mlp_ready ? SPLIT_LIN2 : 0);
    if ((e->split & SPLIT_LIN2) && !e->mx_mlp_ready) e->split &= ~SPLIT_LIN2;          // no MX kernel for these shapes (or lo_format 0): bit ignored
    if (e->split & (SPLIT_ATTN_ANY | SPLIT_MLP | SPLIT_LIN2)) {
        CK(e, dalloc(e, &e->Ylo, M * D));
        if (e->split & SPLIT_MLP) CK(e, dalloc(e, &e->F32T, M * 4 * D));      // the generic attention-side route allocates it on first use
        if (e->split & SPLIT_ATTN_ANY) CK(e, dalloc(e, &e->AOlo, M * D));
        if (e->mx_mlp_ready) {
            for (int h = 0; h < 2; ++h) {
                CK(e, dalloc(e, &e->H4[h], M * e->mx_kp_lin2 / 2)); CK(e, dalloc(e, &e->SH4[h], mx_scale_bytes((int)M, e->mx_kp_lin2, false)));
                if (!e->Y4[h]) { CK(e, dalloc(e, &e->Y4[h], M * D / 2)); CK(e, dalloc(e, &e->SY4[h], mx_scale_bytes((int)M, D, false))); }
            }
        }
        if (e->mx_ready) {
            for (int h = 0; h < 2; ++h) {
                if (!e->Y4[h]) {
                CK(e, dalloc(e, &e->Y4[h], M * D / 2)); CK(e, dalloc(e, &e->SY4[h], mx_scale_bytes((int)M, D, false)));
                }
                CK(e, dalloc(e, &e->AO4[h], M * e->mx_kp_proj / 2)); CK(e, dalloc(e, &e->SAO4[h], mx_scale_bytes((int)M, e->mx_kp_proj, false)));
            }
        }
        if (e->split & SPLIT_MLP) CK(e, dalloc(e, &e->Hlo, M * 4 * D));
    }
    size_t hsz = M * 4 * D;
    if (M * 9 * C * 2 > hsz) hsz = M * 9 * C * 2;      // neck im2col, hi + lo
    if (M * 768 > hsz) hsz = M * 768;
    CK(e, dalloc(e, &e->H, hsz));
    CK(e, dalloc(e, &e->N1, M * C));
    CK(e, dalloc(e, &e->N1e, M * C));
    CK(e, dalloc(e, &e->EMB, M * C));
    CK(e, dalloc(e, &e->K0F, (size_t)c.max_images * tokens * C)); CK(e, dalloc(e, &e->K0E, (size_t)c.max_images * tokens * C));
    CK(e, dalloc(e, &e->KVQ0, (size_t)c.max_images * tokens * 3 * (C / 2)));
    if ((rc = grow_decode_workspaces(e, e->decode_prompts))) return rc;      // every per-prompt decoder workspace
    CK(e, hipStreamSynchronize(s));
    e->dec = dec_weights(e);       // after every to_et(..., free_f32 = true): no freed tensor is resolved
    audit_build_sites(e);
    e->finalized = true;
    return SAMRS_OK;
}

int samrs_get_slot_info(const samrs_engine_t* e, int slot, int32_t* is_set, int32_t* split, int32_t* split_depth) {
    if (!e) return SAMRS_ERR_BAD_ARG;
    if (slot < 0 || slot >= e->cfg.max_images) return SAMRS_ERR_CAPACITY;
    if (is_set) *is_set = e->slot_set[slot];
    if (split) *split = e->slot_set[slot] ? e->slot_split[slot] : 0;
    if (split_depth) *split_depth = e->slot_set[slot] ? e->slot_depth[slot] : 0;
    return SAMRS_OK;
}

int samrs_reset_image(samrs_engine_t* e, int slot) {
    if (!e) return SAMRS_ERR_BAD_ARG;
    if (slot < 0 || slot >= e->cfg.max_images) return fail(e, SAMRS_ERR_CAPACITY, "slot out of range");
    e->slot_set[slot] = 0;
    return SAMRS_OK;
}

// per-engine options (engine_state.h: the list above enum SPLIT_* and the comments of the samrs_engine fields)
int samrs_set_option(samrs_engine_t* e, const char* name, int value) {
    if (!e || !name) return SAMRS_ERR_BAD_ARG;
    const std::string n(name);
    if (n == "decoder_fusion") e->decoder_fusion = value != 0;
    else if (n == "ln_fold") {
        if (value && !gemm_has_experiments())
            return fail(e, SAMRS_ERR_BAD_ARG, "ln_fold: the folded LayerNorm (measured slower: DESIGN.md 6) is built with make EXPERIMENTS=1 only");
        e->ln_fold = value != 0;
    }
    else if (n == "split") {
        if (e->finalized && (value & (SPLIT_ATTN_ANY | SPLIT_MLP | SPLIT_LIN2) & ~e->split_ready))
            return fail(e, SAMRS_ERR_BAD_ARG, "split bits 16 / 32 / 64 / 128 (block GEMMs) need their lo weights: set them before the weights are "
                                              "finalized (SAMRS_SPLIT or options={'split': ...})");
        e->split = value & SPLIT_ALL;
    }
    else if (n == "gemm_variant") e->gemm_variant = value;
    else if (n == "decode_prompts") {
        const long long prod = (long long)e->cfg.max_images * e->cfg.max_prompts;
        const int lo = e->cfg.max_prompts, lim = prod < DECODE_PROMPTS_LIMIT ? (int)prod : DECODE_PROMPTS_LIMIT, hi = lim > lo ? lim : lo;
        if (value < lo || value > hi)
            return fail(e, SAMRS_ERR_BAD_ARG, "decode_prompts=%d is outside [%d, %d]: from max_prompts to max_images x max_prompts = %lld, "
                                              "at most %d (the index range of the decoder kernels)", value, lo, hi, prod, DECODE_PROMPTS_LIMIT);
        if (e->finalized) {          // before that, samrs_finalize_weights allocates at the value set here
            ON_DEVICE(e);
            const int rc = grow_decode_workspaces(e, value);
            if (rc != SAMRS_OK) return rc;
        }
        e->decode_prompts = value;
    }
    else if (n == "upscaler_fused") e->upscaler_fused = value != 0;
    else if (n == "split_passes") e->split_passes = value != 0;
    else if (n == "split_depth") e->split_depth = value > 0 ? value : 0;
    else if (n == "allow_reduced") e->allow_reduced = value != 0;
    else if (n == "gelu_fast") e->gelu_fast = value < 0 ? -1 : (value != 0);
    else if (n == "ln_tail") e->ln_tail = value > 0;
    else if (n == "operand_pad") e->operand_pad_on = value != 0;
    else if (n == "outlier_cols") e->outlier_on = value & 7;
    else if (n == "outlier_ratio_pct") {
        if (e->finalized) return fail(e, SAMRS_ERR_BAD_ARG, "outlier_ratio_pct: the columns are picked when the weights are finalized; set it before");
        if (value < 101) return fail(e, SAMRS_ERR_BAD_ARG, "outlier_ratio_pct must exceed 100 (a column's score as a percentage of the median score)");
        e->outlier_ratio_pct = value;
    }
    else if (n == "range_check") {
        if (value < 0 || value > 2) return fail(e, SAMRS_ERR_BAD_ARG, "range_check is 0 (off), 1 (count) or 2 (count, and samrs_set_images fails)");
        if (value && !e->range_counter) {
            ON_DEVICE(e);
            CK(e, dalloc(e, &e->range_counter, 1));
            CK(e, hipMemset(e->range_counter, 0, sizeof(unsigned long long)));
        }
        if (value == 2 && e->range_check != 2 && e->range_counter) {
            // mode 2 fails the pass that ADDS to the counter: start from what mode 1 has counted so far, or a clean image would be blamed
            ON_DEVICE(e);
            CK(e, hipDeviceSynchronize());
            CK(e, hipMemcpy(&e->range_seen, e->range_counter, sizeof(unsigned long long), hipMemcpyDeviceToHost));
        }
        e->range_check = value;
    }
    else if (n == "saturated") {                    // write = reset (any value)
        if (e->range_counter) {
            ON_DEVICE(e);
            CK(e, hipDeviceSynchronize());
            CK(e, hipMemset(e->range_counter, 0, sizeof(unsigned long long)));
        }
        e->range_seen = 0;
    }
    else if (n == "range_profile") {
        if (value < 0 || value > 2) return fail(e, SAMRS_ERR_BAD_ARG, "range_profile is 0 (off), 1 (range profile per site) or 2 (and column statistics)");
        e->range_profile = value;
        if (!value) e->audit_passes = 0;
    }
    else if (n == "audit_passes") {
        if (value < 0) return fail(e, SAMRS_ERR_BAD_ARG, "audit_passes is the number of encoder passes to profile (0 stops a running audit)");
        if (value > 0) {
            ON_DEVICE(e);
            const int rc = audit_reset(e);
            if (rc != SAMRS_OK) return rc;
            e->range_profile = 2;
        } else if (e->audit_passes > 0) e->range_profile = 0;
        e->audit_passes = value;
    }
    else if (n == "lo_format") {
        if (value != 0 && value != 4) return fail(e, SAMRS_ERR_BAD_ARG, "lo_format is 0 (f16 lo terms) or 4 (MXFP4 lo terms)");
        if (value == 4 && e->finalized && !e->mx_ready && !e->mx_mlp_ready)
            return fail(e, SAMRS_ERR_BAD_ARG, "lo_format 4 needs the fp4 weight copies: set it (and a block-GEMM split bit) before the weights are "
                                              "finalized; it covers the attention-side split of models whose block GEMMs fit the 256 x 320 tile (ViT-H)");
        e->lo_format = value;
    }
    else return fail(e, SAMRS_ERR_BAD_ARG, "unknown option %s", name);
    return SAMRS_OK;
}
int samrs_get_option(const samrs_engine_t* e, const char* name, int* value) {
    if (!e || !name || !value) return SAMRS_ERR_BAD_ARG;
    const std::string n(name);
    if (n == "decoder_fusion") *value = e->decoder_fusion;
    else if (n == "ln_fold") *value = e->ln_fold;
    else if (n == "split") *value = e->split;
    else if (n == "gemm_variant") *value = e->gemm_variant;
    else if (n == "decode_prompts") *value = e->decode_prompts;
    else if (n == "decode_kbytes") *value = (int)((e->decode_bytes + 1023) / 1024);     // read-only; KiB: the bytes do not fit an int
    else if (n == "upscaler_fused") *value = e->upscaler_fused;
    else if (n == "split_passes") *value = e->split_passes;
    else if (n == "split_depth") *value = e->split_depth;
    else if (n == "allow_reduced") *value = e->allow_reduced;
    else if (n == "gelu_fast") *value = e->gelu_fast;
    else if (n == "ln_tail") *value = e->ln_tail;
    else if (n == "operand_pad") *value = e->operand_pad_on;
    else if (n == "outlier_cols") *value = e->outlier_on;
    else if (n == "outlier_ratio_pct") *value = e->outlier_ratio_pct;
    else if (n == "outlier_blocks") *value = e->outlier_blocks;       // read-only
    else if (n == "outlier_columns") *value = e->outlier_columns;     // read-only
    else if (n == "outlier_dominant_blocks") *value = e->outlier_dominant_blocks;   // read-only
    else if (n == "range_check") *value = e->range_check;
    else if (n == "saturated") {                    // synchronizes the device: a diagnostic, not a hot-path call
        unsigned long long c = 0;
        if (e->range_counter) {
            DeviceGuard dg(e->device);
            if (dg.status != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
                hipMemcpy(&c, e->range_counter, sizeof(c), hipMemcpyDeviceToHost) != hipSuccess) return SAMRS_ERR_HIP;
        }
        *value = c > 0x7fffffffull ? 0x7fffffff : (int)c;
    }
    else if (n == "range_profile") *value = e->range_profile;
    else if (n == "audit_passes") *value = e->audit_passes;
    else if (n == "lo_format") *value = (e->finalized && !e->mx_ready && !e->mx_mlp_ready) ? 0 : e->lo_format;
    else if (n == "grade_multimask") *value = e->grade_multimask;     // read-only
    else return SAMRS_ERR_BAD_ARG;
    return SAMRS_OK;
}

}  // extern "C"
