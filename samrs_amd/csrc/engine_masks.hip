// engine_masks.hip -- the entry points that work on finished masks, class maps and prompts' pixels and read no model weights: paint,
// selection, ground-truth match, RLE, scene stitching, clean-up, boxes, polygons, quality gate, overlap, COCO AP (bit planes, pair counts,
// matching), PNG, overlays, resampling, rbox mask prompts.
#include <cmath>

#include "engine_state.h"

extern "C" {
int samrs_paint(samrs_engine_t* e, const uint8_t* masks, const int32_t* labels, int n, int h, int w, uint8_t* seg,
                int64_t* areas, int64_t* cpix, int64_t* cins, int n_classes, void* stream) {
    if (!e || !masks || !labels || n < 1 || h < 1 || w < 1) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_paint: bad argument");
    if ((cpix || cins) && !areas) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_paint: class statistics need areas_out");
    ON_DEVICE(e);
    CK(e, launch_paint(masks, labels, n, h, w, seg, (unsigned long long*)areas, (unsigned long long*)cpix,
                       (unsigned long long*)cins, n_classes, (hipStream_t)stream));
    return SAMRS_OK;
}

int samrs_select_best(samrs_engine_t* e, const uint8_t* masks, const float* iou, int n, int n_sel, int h, int w, uint8_t* best_out,
                      float* quality_out, int64_t* areas_out, void* stream) {
    if (!e || !masks || !iou || !best_out || !quality_out || !areas_out || n < 1 || n_sel < 1 || h < 1 || w < 1)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_select_best: bad argument");
    ON_DEVICE(e);
    CK(e, launch_select_best(masks, iou, n, n_sel, h, w, best_out, quality_out, (unsigned long long*)areas_out, (hipStream_t)stream));
    return SAMRS_OK;
}
int samrs_gt_match(samrs_engine_t* e, const uint8_t* masks, int n, int h, int w, const uint8_t* label_rgb, const uint8_t* colors,
                   int64_t* inter_out, int64_t* gt_area_out, uint8_t* gt_masks_out, void* stream) {
    if (!e || !masks || !label_rgb || !colors || !inter_out || !gt_area_out || n < 1 || h < 1 || w < 1)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_gt_match: bad argument");
    if ((long long)h * w >= (1ll << 30)) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_gt_match: h * w = %lld must stay below 2^30", (long long)h * w);
    ON_DEVICE(e);
    CK(e, launch_gt_match(masks, n, h, w, label_rgb, colors, (unsigned long long*)inter_out, (unsigned long long*)gt_area_out, gt_masks_out,
                          (hipStream_t)stream));
    return SAMRS_OK;
}

// COCO RLE strings of n masks, packed behind *cursor into `out` (see samrs_hip.h)
int samrs_rle_encode(samrs_engine_t* e, const uint8_t* masks, int n, int h, int w, uint8_t* out, int64_t out_capacity,
                     int64_t* cursor, int64_t* table, void* stream) {
    if (!e || !masks || !out || !cursor || !table || n < 1 || h < 1 || w < 1 || out_capacity < 16)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_rle_encode: bad argument");
    if ((size_t)h * w >= (1ull << 30) || w > 8192)
        return fail(e, SAMRS_ERR_BAD_SHAPE, "samrs_rle_encode: mask too large (h * w must be < 2^30, w <= 8192)");
    ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const int chunk = 32;                               // masks per pass: bounds the scratch (5.3 MB per 1024^2 mask)
    const size_t need = rle_scratch_bytes(n < chunk ? n : chunk, h, w);
    CK(e, scratch_reserve(e->rle_scratch, need, s));
    for (int off = 0; off < n; off += chunk) {
        const int m = n - off < chunk ? n - off : chunk;
        CK(e, launch_rle_encode(masks + (size_t)off * h * w, m, h, w, e->rle_scratch.p, out, (long long)out_capacity,
                                (long long*)cursor, (long long*)table + (size_t)off * 3, s));
    }
    return SAMRS_OK;
}

// the inverse: n COCO RLE strings decoded to row-major 0 / 1 bytes, with a status per mask (see samrs_hip.h)
int samrs_rle_decode(samrs_engine_t* e, const uint8_t* strings, int64_t strings_bytes, const int64_t* table, int n, int h, int w,
                     uint8_t* masks_out, int64_t* areas_out, int32_t* status_out, void* stream) {
    if (!e || n < 0 || h < 1 || w < 1 || strings_bytes < 0 || (n > 0 && (!strings || !table || !masks_out || !status_out)))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_rle_decode: bad argument");
    if ((size_t)h * w >= (1ull << 30) || strings_bytes >= (1ll << 31))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_rle_decode: too large (h * w must be < 2^30, strings_bytes < 2^31)");
    if (n == 0) return SAMRS_OK;
    ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    // masks per pass: as many as keep the bit matrix below 64 MiB (rle_decode_max_batch() at most), one at least
    const size_t per = ((size_t)(h + 31) / 32) * w * 4;
    int chunk = (int)(((size_t)64 << 20) / per);
    chunk = chunk < 1 ? 1 : (chunk > rle_decode_max_batch() ? rle_decode_max_batch() : chunk);
    const size_t need = rle_decode_scratch_bytes(n < chunk ? n : chunk, h, w, (long long)strings_bytes);
    CK(e, scratch_reserve(e->rle_decode_scratch, need, s));
    for (int off = 0; off < n; off += chunk) {
        const int m = n - off < chunk ? n - off : chunk;
        CK(e, launch_rle_decode(strings, (long long)strings_bytes, (const long long*)table + (size_t)off * 3, m, h, w,
                                e->rle_decode_scratch.p, masks_out + (size_t)off * h * w, areas_out ? (long long*)areas_out + off : nullptr,
                                status_out + off, s));
    }
    return SAMRS_OK;
}

// scene mode (see samrs_hip.h): one window's masks into the scene's rank map, the map into the class map, and the window's masks
// as COCO RLE strings in the scene's frame
int samrs_scene_claim(samrs_engine_t* e, const uint8_t* masks, const int32_t* ranks, const int32_t* labels, int n, int h, int w,
                      int x0, int y0, int H, int W, int32_t* order, int64_t* areas, int64_t* cpix, int64_t* cins, int n_classes,
                      void* stream) {
    if (!e || (n > 0 && (!masks || !ranks)) || !order || n < 0 || h < 1 || w < 1 || H < 1 || W < 1)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_scene_claim: bad argument");
    if (x0 < 0 || y0 < 0 || x0 > W - w || y0 > H - h)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_scene_claim: window (%d, %d, %d, %d) is not inside the %d x %d scene", x0, y0, w, h, H, W);
    if ((cpix || cins) && (!areas || !labels)) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_scene_claim: class statistics need areas_out and labels");
    ON_DEVICE(e);
    CK(e, launch_scene_claim(masks, ranks, labels, n, h, w, x0, y0, H, W, order, (unsigned long long*)areas, (unsigned long long*)cpix,
                             (unsigned long long*)cins, n_classes, (hipStream_t)stream));
    return SAMRS_OK;
}
int samrs_scene_resolve(samrs_engine_t* e, const int32_t* order, const int32_t* labels_by_rank, int n_ranks, int H, int W, uint8_t* seg,
                        void* stream) {
    if (!e || !order || !seg || n_ranks < 0 || (n_ranks > 0 && !labels_by_rank) || H < 1 || W < 1)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_scene_resolve: bad argument");
    ON_DEVICE(e);
    CK(e, launch_scene_resolve(order, labels_by_rank, n_ranks, H, W, seg, (hipStream_t)stream));
    return SAMRS_OK;
}
int samrs_rle_encode_placed(samrs_engine_t* e, const uint8_t* masks, int n, int h, int w, int x0, int y0, int H, int W, uint8_t* out,
                            int64_t out_capacity, int64_t* cursor, int64_t* table, void* stream) {
    if (!e || (n > 0 && (!masks || !table)) || !out || !cursor || n < 0 || h < 1 || w < 1 || H < 1 || W < 1 || out_capacity < 16)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_rle_encode_placed: bad argument");
    if (x0 < 0 || y0 < 0 || x0 > W - w || y0 > H - h)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_rle_encode_placed: window (%d, %d, %d, %d) is not inside the %d x %d canvas", x0, y0, w, h, H, W);
    if ((size_t)H * W >= (1ull << 30) || w >= 8192)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_rle_encode_placed: canvas or window too large (H * W must be < 2^30, w < 8192)");
    if (n == 0) return SAMRS_OK;
    ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    // masks per pass: as many as keep the scratch below 256 MiB (32 at most, as samrs_rle_encode), one at least
    const size_t per = rle_placed_scratch_bytes(1, h, w, x0, H, W);
    int chunk = (int)(((size_t)256 << 20) / per);
    chunk = chunk < 1 ? 1 : (chunk > 32 ? 32 : chunk);
    const size_t need = rle_placed_scratch_bytes(n < chunk ? n : chunk, h, w, x0, H, W);
    CK(e, scratch_reserve(e->rle_scratch, need, s));
    for (int off = 0; off < n; off += chunk) {
        const int m = n - off < chunk ? n - off : chunk;
        CK(e, launch_rle_encode_placed(masks + (size_t)off * h * w, m, h, w, x0, y0, H, W, e->rle_scratch.p, out, (long long)out_capacity,
                                       (long long*)cursor, (long long*)table + (size_t)off * 3, s));
    }
    return SAMRS_OK;
}

// small islands and holes of n masks removed in place (see samrs_hip.h)
int samrs_clean_masks(samrs_engine_t* e, uint8_t* masks, int n, int h, int w, int min_area, int mode, int64_t* areas_out,
                      int64_t* changed_out, void* stream) {
    if (!e || !masks || n < 1 || h < 1 || w < 1 || min_area < 1 || mode < SAMRS_REGION_HOLES || mode > SAMRS_REGION_BOTH)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_clean_masks: bad argument");
    if ((size_t)h * w >= (1ull << 30)) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_clean_masks: h * w = %lld must stay below 2^30", (long long)h * w);
    ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const int chunk = REGION_CHUNK;                     // masks per pass: bounds the scratch (8 MiB per 1024^2 mask)
    const size_t need = region_scratch_bytes(n < chunk ? n : chunk, h, w);
    CK(e, scratch_reserve(e->region_scratch, need, s));
    for (int off = 0; off < n; off += chunk) {
        const int m = n - off < chunk ? n - off : chunk;
        CK(e, launch_clean_masks(masks + (size_t)off * h * w, m, h, w, min_area, mode, e->region_scratch.p,
                                 areas_out ? (long long*)areas_out + off : nullptr, changed_out ? (long long*)changed_out + off : nullptr, s));
    }
    return SAMRS_OK;
}

// tight hbox, minimum-area rbox and record of n masks (see samrs_hip.h)
int samrs_mask_boxes(samrs_engine_t* e, const uint8_t* masks, int n, int h, int w, int x0, int y0, int32_t* hbox_out, float* rbox_out,
                     int64_t* record_out, void* stream) {
    if (!e || !masks || n < 0) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_mask_boxes: bad argument");
    if (!mask_boxes_shape_ok(h, w, x0, y0))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_mask_boxes: %d x %d masks at (%d, %d): h, w must be 1..8192 and x0 + w, y0 + h <= 32768",
                    h, w, x0, y0);
    if (n == 0 || (!hbox_out && !rbox_out && !record_out)) return SAMRS_OK;
    ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const int cap = (int)(((size_t)64 << 20) / mask_boxes_scratch_bytes(1, h));      // masks per pass: the scratch stays below 64 MiB
    const int chunk = n < cap ? n : cap;
    const size_t need = mask_boxes_scratch_bytes(chunk, h);
    CK(e, scratch_reserve(e->box_scratch, need, s));
    for (int off = 0; off < n; off += chunk) {
        const int m = n - off < chunk ? n - off : chunk;
        CK(e, launch_mask_row_extents(masks + (size_t)off * h * w, m, h, w, (int32_t*)e->box_scratch.p, s));
        CK(e, launch_mask_hull_rect((const int32_t*)e->box_scratch.p, m, h, x0, y0, hbox_out ? hbox_out + (size_t)off * 4 : nullptr,
                                    rbox_out ? rbox_out + (size_t)off * 8 : nullptr,
                                    record_out ? (long long*)record_out + (size_t)off * 8 : nullptr, nullptr, 0, nullptr, s));
    }
    return SAMRS_OK;
}

// the outlines of n masks as polygons behind a device-side cursor (see samrs_hip.h)
int samrs_mask_polygons(samrs_engine_t* e, const uint8_t* masks, int n, int h, int w, int x0, int y0, int max_edges, int32_t* vertices,
                        int64_t vertex_capacity, int32_t* rings, int64_t ring_capacity, int64_t* cursor, int64_t* table, void* stream) {
    if (!e || !masks || !table || !cursor || !vertices || !rings || n < 0 || max_edges < 4 || vertex_capacity < 0 || ring_capacity < 0)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_mask_polygons: bad argument");
    if (!mask_polygons_shape_ok(h, w, x0, y0))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_mask_polygons: %d x %d masks at (%d, %d): h, w must be 1..8192, x0 + w, y0 + h <= 32768 "
                    "and h * w < 2^30", h, w, x0, y0);
    {   // what samrs_simplify_polygons may later be handed: the same pair of buffers keeps one entry, with its latest capacities
        auto& seen = e->poly_seen;
        for (size_t i = 0; i < seen.size(); ++i)
            if (seen[i].vertices == vertices && seen[i].rings == rings) { seen.erase(seen.begin() + i); break; }
        if (seen.size() >= 16) seen.erase(seen.begin());
        seen.push_back({vertices, rings, (long long)vertex_capacity, (long long)ring_capacity});
    }
    if (n == 0) return SAMRS_OK;
    ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    // masks per pass: as many as keep the scratch at or below 256 MiB (n masks need at most n times one mask's bytes), one at least
    size_t cap = ((size_t)256 << 20) / mask_polygons_scratch_bytes(1, h, w, max_edges);
    cap = cap < 1 ? 1 : (cap > 4096 ? 4096 : cap);
    const int step = (size_t)n < cap ? n : (int)cap;
    const size_t need = mask_polygons_scratch_bytes(step, h, w, max_edges);
    CK(e, scratch_reserve(e->poly_scratch, need, s));
    for (int off = 0; off < n; off += step) {
        const int m = n - off < step ? n - off : step;
        CK(e, launch_mask_polygons(masks + (size_t)off * h * w, m, h, w, x0, y0, max_edges, e->poly_scratch.p, vertices,
                                   (long long)vertex_capacity, rings, (long long)ring_capacity, (long long*)cursor,
                                   (long long*)table + (size_t)off * 5, s));
    }
    return SAMRS_OK;
}

// the traced rings of n rows simplified in place (see samrs_hip.h)
int samrs_simplify_polygons(samrs_engine_t* e, int32_t* vertices, int32_t* rings, int64_t* table, int n, int eps_q, int64_t* cursor,
                            void* stream) {
    if (!e || !vertices || !rings || !table || !cursor || n < 0) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_simplify_polygons: bad argument");
    if (eps_q < 1 || eps_q > POLYGON_SIMPLIFY_EPS_MAX)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_simplify_polygons: eps_q = %d must lie in 1..%d (sixteenths of a pixel)", eps_q,
                    POLYGON_SIMPLIFY_EPS_MAX);
    if (n == 0) return SAMRS_OK;
    const samrs_engine::PolyBuffers* buf = nullptr;
    for (const auto& b : e->poly_seen)
        if (b.vertices == vertices && b.rings == rings) buf = &b;
    if (!buf)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_simplify_polygons: samrs_mask_polygons of this handle has not traced into these buffers "
                    "(their capacities are not known)");
    ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    CK(e, scratch_reserve(e->poly_scratch, polygon_simplify_scratch_bytes(n, buf->vcap, buf->rcap), s));
    CK(e, launch_polygon_simplify(vertices, rings, (long long*)table, n, eps_q, buf->vcap, buf->rcap, e->poly_scratch.p, (long long*)cursor, s));
    return SAMRS_OK;
}

// the rings of n table rows filled even-odd at the pixel centres, and counted against ref (see samrs_hip.h)
int samrs_fill_polygons(samrs_engine_t* e, const int32_t* vertices, const int32_t* rings, const int64_t* table, int n, int h, int w,
                        int x0, int y0, uint8_t* masks_out, const uint8_t* ref, int64_t* counts_out, void* stream) {
    if (!e || !vertices || !rings || !table || n < 0) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_fill_polygons: bad argument");
    if (!masks_out && !counts_out) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_fill_polygons: masks_out and counts_out are both null");
    if (!mask_boxes_shape_ok(h, w, x0, y0))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_fill_polygons: %d x %d masks at (%d, %d): h, w must be 1..8192 and x0 + w, y0 + h <= 32768",
                    h, w, x0, y0);
    if (n == 0) return SAMRS_OK;
    ON_DEVICE(e);
    CK(e, launch_fill_polygons(vertices, rings, (const long long*)table, n, h, w, x0, y0, masks_out, ref, (long long*)counts_out,
                               (hipStream_t)stream));
    return SAMRS_OK;
}

// threshold counts of n masks straight from their 256^2 logits (see samrs_hip.h)
int samrs_score_masks(samrs_engine_t* e, const float* lowres, int n, int in_h, int in_w, int orig_h, int orig_w, float offset,
                      const float* boxes, int64_t* counts_out, void* stream) {
    if (!e || !lowres || !counts_out || n < 0) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_score_masks: bad argument");
    if (!(offset >= 0.f) || !std::isfinite(offset))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_score_masks: offset must be finite and >= 0");
    const int img = e->cfg.img_size;
    if (in_h < 1 || in_w < 1 || in_h > img || in_w > img || (in_h != img && in_w != img) || orig_h < 1 || orig_w < 1 ||
        (long long)orig_h * orig_w >= (1ll << 31))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_score_masks: input %d x %d (long side must be %d), output %d x %d (h * w < 2^31)", in_h,
                    in_w, img, orig_h, orig_w);
    if (n == 0) return SAMRS_OK;
    ON_DEVICE(e);
    CK(e, launch_score_masks(lowres, n, in_h, in_w, orig_h, orig_w, img, offset, boxes, (unsigned long long*)counts_out,
                             (hipStream_t)stream));
    return SAMRS_OK;
}

// the quality gate: keep flags from the counts, dropped masks zeroed in place (see samrs_hip.h)
int samrs_filter_masks(samrs_engine_t* e, uint8_t* masks, int n, int h, int w, const int64_t* counts, const float* iou,
                       float min_stability, float min_pred_iou, float min_inside, uint8_t* keep_out, void* stream) {
    if (!e || !masks || !counts || !keep_out || n < 0 || h < 1 || w < 1) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_filter_masks: bad argument");
    if (min_pred_iou > 0.f && !iou) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_filter_masks: min_pred_iou > 0 needs iou");
    if (std::isnan(min_stability) || std::isnan(min_pred_iou) || std::isnan(min_inside))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_filter_masks: a threshold is NaN");
    if (n == 0) return SAMRS_OK;
    ON_DEVICE(e);
    CK(e, launch_filter_masks(masks, n, (long)h * w, (const long long*)counts, iou, min_stability, min_pred_iou, min_inside, keep_out,
                              (hipStream_t)stream));
    return SAMRS_OK;
}

// one instance per pixel: contested pixels given to one mask, cleared in the others, in place (see samrs_hip.h)
int samrs_resolve_overlaps(samrs_engine_t* e, uint8_t* masks, int n, int h, int w, int rule, const float* lowres, int in_h, int in_w,
                           const int64_t* priority, int32_t* owner_out, int64_t* before_out, int64_t* removed_out, void* stream) {
    if (!e || !masks || n < 0) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_resolve_overlaps: bad argument");
    if (rule != SAMRS_OVERLAP_LOGIT && rule != SAMRS_OVERLAP_SMALLEST && rule != SAMRS_OVERLAP_PRIORITY)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_resolve_overlaps: unknown rule %d", rule);
    if (rule == SAMRS_OVERLAP_LOGIT && !lowres) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_resolve_overlaps: rule LOGIT needs lowres");
    if (rule == SAMRS_OVERLAP_PRIORITY && !priority) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_resolve_overlaps: rule PRIORITY needs priority");
    const int img = e->cfg.img_size;
    if (h < 1 || w < 1 || (long long)h * w >= (1ll << 31))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_resolve_overlaps: masks %d x %d (h, w >= 1, h * w < 2^31)", h, w);
    if (lowres && (in_h < 1 || in_w < 1 || in_h > img || in_w > img || (in_h != img && in_w != img)))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_resolve_overlaps: input %d x %d (long side must be %d)", in_h, in_w, img);
    if (n == 0) return SAMRS_OK;
    ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* before = (unsigned long long*)before_out;
    if (rule == SAMRS_OVERLAP_SMALLEST && !before) {
        CK(e, scratch_reserve(e->overlap_scratch, sizeof(unsigned long long) * (size_t)n, s));
        before = (unsigned long long*)e->overlap_scratch.p;
    }
    if (before) CK(e, launch_mask_areas(masks, n, h, w, before, s));
    const long long* prim = rule == SAMRS_OVERLAP_PRIORITY ? (const long long*)priority
                          : rule == SAMRS_OVERLAP_SMALLEST ? (const long long*)before : nullptr;
    CK(e, launch_resolve_overlaps(masks, n, h, w, prim, rule == SAMRS_OVERLAP_SMALLEST ? 1 : 0, lowres, in_h, in_w, img, owner_out,
                                  (unsigned long long*)removed_out, s));
    return SAMRS_OK;
}

// COCO mask AP (see samrs_hip.h): bit planes of masks / of a label image's instances, pairwise counts, the greedy matching
int samrs_mask_pack_bits(samrs_engine_t* e, const uint8_t* masks, int n, int h, int w, uint64_t* planes_out, void* stream) {
    if (!e || !masks || !planes_out || n < 0) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_mask_pack_bits: bad argument");
    if (h < 1 || w < 1 || (long long)h * w >= (1ll << 30))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_mask_pack_bits: masks %d x %d (h, w >= 1, h * w < 2^30)", h, w);
    if (n == 0) return SAMRS_OK;
    ON_DEVICE(e);
    CK(e, launch_pack_bits(masks, n, h, w, (unsigned long long*)planes_out, (hipStream_t)stream));
    return SAMRS_OK;
}
int samrs_label_pack_bits(samrs_engine_t* e, const uint8_t* label_rgb, const uint8_t* colors, int n, int h, int w, uint64_t* planes_out,
                          void* stream) {
    if (!e || !label_rgb || !colors || !planes_out || n < 0) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_label_pack_bits: bad argument");
    if (h < 1 || w < 1 || (long long)h * w >= (1ll << 30))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_label_pack_bits: label image %d x %d (h, w >= 1, h * w < 2^30)", h, w);
    if (n == 0) return SAMRS_OK;
    ON_DEVICE(e);
    CK(e, launch_label_pack_bits(label_rgb, colors, n, h, w, (unsigned long long*)planes_out, (hipStream_t)stream));
    return SAMRS_OK;
}
int samrs_mask_pair_counts(samrs_engine_t* e, const uint64_t* a, int na, const uint64_t* b, int nb, int64_t words, int64_t* inter_out,
                           int64_t* area_a_out, int64_t* area_b_out, void* stream) {
    if (!e || na < 0 || nb < 0 || (na > 0 && !a) || (nb > 0 && !b) || (na > 0 && nb > 0 && !inter_out))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_mask_pair_counts: bad argument");
    if (words < 1 || words > (1ll << 24))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_mask_pair_counts: %lld words per plane (1 .. 2^24)", (long long)words);
    if ((na + 63) / 64 > 65535 || (nb + 63) / 64 > 65535) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_mask_pair_counts: too many planes");
    if (na == 0 && nb == 0) return SAMRS_OK;
    ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    if (na > 0 && area_a_out) CK(e, launch_bit_areas((const unsigned long long*)a, na, (long)words, (unsigned long long*)area_a_out, s));
    if (nb > 0 && area_b_out) CK(e, launch_bit_areas((const unsigned long long*)b, nb, (long)words, (unsigned long long*)area_b_out, s));
    if (na > 0 && nb > 0)
        CK(e, launch_pair_counts((const unsigned long long*)a, na, (const unsigned long long*)b, nb, (long)words,
                                 (unsigned long long*)inter_out, s));
    return SAMRS_OK;
}
// samrs_coco_match (band triple null) and samrs_coco_match_min (`with_min`: the triple is required like the first one)
static int coco_match_entry(const char* who, bool with_min, samrs_engine_t* e, const int64_t* inter, const int64_t* area_d,
                            const int64_t* area_g, const int64_t* inter_b, const int64_t* area_db, const int64_t* area_gb, const float* scores,
                            int scores_on_host, int nd, int ng, const double* thresholds, int n_thresholds, const double* area_ranges,
                            int n_ranges, int max_det, int32_t* order_out, int32_t* match_out, uint8_t* dt_ignore_out, int32_t* n_valid_out,
                            int32_t* n_kept_out, void* stream) {
    if (with_min && ((nd > 0 && !area_db) || (ng > 0 && !area_gb) || (nd > 0 && ng > 0 && !inter_b)))
        return fail(e, SAMRS_ERR_BAD_ARG, "%s: bad argument", who);
    if (!e || nd < 0 || ng < 0 || !thresholds || !area_ranges || !order_out || !match_out || !dt_ignore_out || !n_valid_out || !n_kept_out ||
        (nd > 0 && (!scores || !area_d)) || (ng > 0 && !area_g) || (nd > 0 && ng > 0 && !inter))
        return fail(e, SAMRS_ERR_BAD_ARG, "%s: bad argument", who);
    if (n_thresholds < 1 || n_thresholds > COCO_MAX_THRESHOLDS || n_ranges < 1 || n_ranges > COCO_MAX_RANGES || max_det < 1 ||
        max_det > COCO_MAX_DET)
        return fail(e, SAMRS_ERR_BAD_ARG, "%s: %d thresholds (1..%d), %d area ranges (1..%d), max_det %d (1..%d)", who, n_thresholds,
                    COCO_MAX_THRESHOLDS, n_ranges, COCO_MAX_RANGES, max_det, COCO_MAX_DET);
    CocoMatchParams P{};
    for (int t = 0; t < n_thresholds; ++t) {
        if (std::isnan(thresholds[t])) return fail(e, SAMRS_ERR_BAD_ARG, "%s: threshold %d is NaN", who, t);
        P.bar[t] = std::fmin(thresholds[t], 1.0 - 1e-10);
    }
    for (int a = 0; a < n_ranges; ++a) {
        P.lo[a] = area_ranges[2 * a];
        P.hi[a] = area_ranges[2 * a + 1];
        if (std::isnan(P.lo[a]) || std::isnan(P.hi[a])) return fail(e, SAMRS_ERR_BAD_ARG, "%s: area range %d is NaN", who, a);
    }
    if (scores_on_host)
        for (int d = 0; d < nd; ++d)
            if (std::isnan(scores[d])) return fail(e, SAMRS_ERR_BAD_ARG, "%s: score %d is NaN", who, d);
    ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t flags = coco_match_scratch_bytes(ng, n_thresholds, n_ranges);
    CK(e, scratch_reserve(e->ap_scratch, flags + (scores_on_host ? sizeof(float) * (size_t)nd : 0), s));
    const float* dev_scores = scores;
    if (scores_on_host && nd > 0) {
        float* staged = (float*)((char*)e->ap_scratch.p + flags);
        CK(e, hipMemcpyAsync(staged, scores, sizeof(float) * (size_t)nd, hipMemcpyHostToDevice, s));
        dev_scores = staged;
    }
    CK(e, launch_coco_match((const long long*)inter, (const long long*)area_d, (const long long*)area_g,
                            with_min ? (const long long*)inter_b : nullptr, with_min ? (const long long*)area_db : nullptr,
                            with_min ? (const long long*)area_gb : nullptr, dev_scores, nd, ng, P, n_thresholds, n_ranges, max_det,
                            e->ap_scratch.p, order_out, match_out, dt_ignore_out, n_valid_out, n_kept_out, s));
    return SAMRS_OK;
}

int samrs_coco_match(samrs_engine_t* e, const int64_t* inter, const int64_t* area_d, const int64_t* area_g, const float* scores,
                     int scores_on_host, int nd, int ng, const double* thresholds, int n_thresholds, const double* area_ranges,
                     int n_ranges, int max_det, int32_t* order_out, int32_t* match_out, uint8_t* dt_ignore_out, int32_t* n_valid_out,
                     int32_t* n_kept_out, void* stream) {
    return coco_match_entry("samrs_coco_match", false, e, inter, area_d, area_g, nullptr, nullptr, nullptr, scores, scores_on_host, nd, ng,
                            thresholds, n_thresholds, area_ranges, n_ranges, max_det, order_out, match_out, dt_ignore_out, n_valid_out,
                            n_kept_out, stream);
}
int samrs_coco_match_min(samrs_engine_t* e, const int64_t* inter, const int64_t* area_d, const int64_t* area_g, const int64_t* inter_b,
                         const int64_t* area_db, const int64_t* area_gb, const float* scores, int scores_on_host, int nd, int ng,
                         const double* thresholds, int n_thresholds, const double* area_ranges, int n_ranges, int max_det,
                         int32_t* order_out, int32_t* match_out, uint8_t* dt_ignore_out, int32_t* n_valid_out, int32_t* n_kept_out,
                         void* stream) {
    return coco_match_entry("samrs_coco_match_min", true, e, inter, area_d, area_g, inter_b, area_db, area_gb, scores, scores_on_host, nd, ng,
                            thresholds, n_thresholds, area_ranges, n_ranges, max_det, order_out, match_out, dt_ignore_out, n_valid_out,
                            n_kept_out, stream);
}

// the boundary bands of n bit planes (see samrs_hip.h)
int samrs_mask_boundary_bits(samrs_engine_t* e, const uint64_t* planes, int n, int h, int w, int d, uint64_t* band_out, void* stream) {
    if (!e || !planes || !band_out || n < 0) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_mask_boundary_bits: bad argument");
    if (h < 1 || w < 1 || (long long)h * w >= (1ll << 30))
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_mask_boundary_bits: masks %d x %d (h, w >= 1, h * w < 2^30)", h, w);
    if (d < 1 || d > 128) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_mask_boundary_bits: d = %d must lie in 1..128", d);
    const size_t words = ((size_t)h * w + 63) / 64, total = words * (size_t)n;
    if (n > 0 && planes < band_out + total && band_out < planes + total)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_mask_boundary_bits: band_out overlaps planes");
    if (n == 0) return SAMRS_OK;
    ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t cap = ((size_t)64 << 20) / (words * sizeof(uint64_t));      // masks per pass: the intermediate planes stay below 64 MiB
    const int chunk = cap < 1 ? 1 : ((size_t)n < cap ? n : (int)cap);
    const bool trivial = w < 2 * d + 1 || h < 2 * d + 1;                     // no square fits: the band is the mask, no intermediate
    if (!trivial) CK(e, scratch_reserve(e->boundary_scratch, mask_boundary_scratch_bytes(chunk, h, w), s));
    for (int off = 0; off < n; off += chunk) {
        const int m = n - off < chunk ? n - off : chunk;
        CK(e, launch_mask_boundary((const unsigned long long*)planes + (size_t)off * words, m, h, w, d,
                                   trivial ? nullptr : e->boundary_scratch.p, (unsigned long long*)band_out + (size_t)off * words, s));
    }
    return SAMRS_OK;
}

// gray + colour PNG files of n class maps, packed behind *cursor into `out` (see samrs_hip.h)
int samrs_png_encode_labels(samrs_engine_t* e, const uint8_t* maps, int n, int h, int w, const uint8_t* lut, uint8_t* out,
                            int64_t out_capacity, int64_t* cursor, int64_t* table, void* stream) {
    if (!e || !maps || !lut || !out || !cursor || !table || n < 1 || h < 1 || w < 1 || out_capacity < 16)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_png_encode_labels: bad argument");
    if (((uintptr_t)out & 15) != 0) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_png_encode_labels: out must be 16-byte aligned");
    if (h > 65536 || w > 65536 || ((size_t)3 * w + 1) * h > 0x7fffffffull)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_png_encode_labels: %d x %d map too large (h, w <= 65536, (3 w + 1) h < 2^31)", h, w);
    ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    const size_t need = png_scratch_bytes(n, h, w);
    CK(e, scratch_reserve(e->png_scratch, need, s));
    CK(e, launch_png_encode(maps, n, h, w, lut, e->png_scratch.p, out, (long long)out_capacity, (long long*)cursor, (long long*)table, s));
    return SAMRS_OK;
}

// visualize.py's overlay of n images with their class maps (see samrs_hip.h)
int samrs_blend_labels(samrs_engine_t* e, const uint8_t* images, const uint8_t* maps, const uint8_t* lut, float alpha, uint8_t* out, int n,
                       int h, int w, void* stream) {
    if (!e || !images || !maps || !lut || !out || out == images || n < 1 || h < 1 || w < 1)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_blend_labels: bad argument");
    if (!(alpha >= 0.f && alpha <= 1.f)) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_blend_labels: alpha = %g must lie in [0, 1]", (double)alpha);
    ON_DEVICE(e);
    CK(e, launch_blend_labels(images, maps, lut, alpha, out, n, h, w, (hipStream_t)stream));
    return SAMRS_OK;
}

// truecolour PNG files of n images, packed behind *cursor into `out` (see samrs_hip.h)
int samrs_png_encode_rgb(samrs_engine_t* e, const uint8_t* rgb, int n, int h, int w, int filter, uint8_t* out, int64_t out_capacity,
                         int64_t* cursor, int64_t* table, void* stream) {
    if (!e || !rgb || !out || !cursor || !table || n < 1 || h < 1 || w < 1 || out_capacity < 16 || filter < -1 || filter > 4)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_png_encode_rgb: bad argument");
    if (((uintptr_t)out & 15) != 0) return fail(e, SAMRS_ERR_BAD_ARG, "samrs_png_encode_rgb: out must be 16-byte aligned");
    if (h > 65536 || w > 65536 || ((size_t)3 * w + 1) * h > 0x7fffffffull)
        return fail(e, SAMRS_ERR_BAD_ARG, "samrs_png_encode_rgb: %d x %d image too large (h, w <= 65536, (3 w + 1) h < 2^31)", h, w);
    ON_DEVICE(e);
    hipStream_t s = (hipStream_t)stream;
    CK(e, scratch_reserve(e->png_rgb_scratch, png_rgb_scratch_bytes(n, h, w), s));
    CK(e, launch_png_encode_rgb(rgb, n, h, w, filter, e->png_rgb_scratch.p, out, (long long)out_capacity, (long long*)cursor,
                                (long long*)table, s));
    return SAMRS_OK;
}

int samrs_resample_pass_u8(const uint8_t* in, uint8_t* out, const int32_t* bounds, const int32_t* coef, int ksize,
                           int in_len, int out_len, int other, int horizontal, void* stream) {
    if (!in || !out || !bounds || !coef || ksize < 1 || in_len < 1 || out_len < 1 || other < 1) return SAMRS_ERR_BAD_ARG;
    KRET(launch_resample_pass(in, out, bounds, coef, ksize, in_len, out_len, other, horizontal, (hipStream_t)stream));
}
int samrs_rbox_mask_prompt(const int32_t* pts, int n, int n_vertices, int h, int w, int th, int tw, int img_size, int out_size,
                           float* out, void* stream) {
    if (!pts || !out) return SAMRS_ERR_BAD_ARG;
    KRET(launch_rbox_prompt(pts, n, n_vertices, h, w, th, tw, img_size, out_size, out, (hipStream_t)stream, SAMRS_FILL_CV2_LE_451));
}
int samrs_rbox_mask_prompt_rule(const int32_t* pts, int n, int n_vertices, int h, int w, int th, int tw, int img_size, int out_size,
                                int fill_rule, float* out, void* stream) {
    if (!pts || !out || (fill_rule != SAMRS_FILL_CV2_LE_451 && fill_rule != SAMRS_FILL_CV2_GE_452)) return SAMRS_ERR_BAD_ARG;
    KRET(launch_rbox_prompt(pts, n, n_vertices, h, w, th, tw, img_size, out_size, out, (hipStream_t)stream, fill_rule));
}
}  // extern "C"
