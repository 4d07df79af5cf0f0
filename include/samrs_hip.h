/*
 * samrs_hip.h -- C ABI of libsamrs_hip.so, the MI355X (gfx950) SAM box->mask engine.
 *
 * This is the drop-in boundary for the ONE hot path of ViTAE-Transformer/SAMRS: what
 * `SamPredictor.set_image()` / `predict_torch()` compute
 * (reference: Generate Dataset/segment_anything/predictor.py:34-90,168-245).
 * Plain pointers + sizes only; no torch types.  All data pointers are DEVICE pointers unless a
 * parameter says otherwise; every entry point that launches work takes the HIP stream to launch
 * on (`hipStream_t` passed as `void*`; NULL = the legacy default stream) and does NOT
 * synchronise -- exactly like the reference, where the sync happens at the caller's `.cpu()`
 * (Generate Dataset/main_sam_hbox_semantic.py:189).
 *
 * One engine handle per GPU per process; a handle is not thread-safe (neither is the
 * reference's stateful SamPredictor, predictor.py:84-90).
 *
 * Return convention: 0 = OK, negative = error code below; `samrs_last_error()` returns the
 * message.  The Python wrapper re-raises the reference's exception types / messages
 * (predictor.py:133-134,213-214: RuntimeError "An image must be set ...").
 */
#ifndef SAMRS_HIP_H
#define SAMRS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAMRS_ABI_VERSION 5

enum samrs_status {
    SAMRS_OK = 0,
    SAMRS_ERR_NOT_SET = -1,      /* predict before set_images (predictor.py:213-214)            */
    SAMRS_ERR_BAD_SHAPE = -2,    /* e.g. long side != 1024 (predictor.py:79-83)                 */
    SAMRS_ERR_BAD_ARG = -3,      /* points without labels (predictor.py:139-141), null ptrs ... */
    SAMRS_ERR_HIP = -4,          /* a HIP runtime call failed                                   */
    SAMRS_ERR_BAD_WEIGHTS = -5,  /* unknown / missing / mis-shaped tensor (strict load,
                                    build_sam.py:103-106)                                       */
    SAMRS_ERR_CAPACITY = -6,     /* more images / prompts than the handle was created for       */
    SAMRS_ERR_PRECISION = -7,    /* multimask predict on an embedding encoded below the mode the
                                    multimask outputs need (see samrs_get_slot_info)            */
    SAMRS_ERR_RANGE = -8         /* option "range_check" = 2: an encoder pass saturated values of
                                    an MFMA operand tensor (f16: |x| >= 65504)                  */
};

/* MFMA operand type.  Accumulation, residual stream, LayerNorm / softmax statistics and the
 * whole token side of the decoder are always fp32. */
enum samrs_precision {
    SAMRS_PREC_BF16 = 0,
    SAMRS_PREC_F16 = 1
};

/* Model hyper-parameters: Generate Dataset/segment_anything/build_sam.py:14-21,37-44,55-98. */
typedef struct samrs_config {
    int32_t embed_dim;               /* 1280 (vit_h) / 1024 (vit_l) / 768 (vit_b)            */
    int32_t depth;                   /* 32 / 24 / 12                                          */
    int32_t num_heads;               /* 16 / 16 / 12                                          */
    int32_t n_global;                /* number of valid entries in global_attn_indexes        */
    int32_t global_attn_indexes[8];  /* blocks that use global attention                      */
    int32_t img_size;                /* 1024                                                  */
    int32_t patch_size;              /* 16                                                    */
    int32_t window_size;             /* 14                                                    */
    int32_t out_chans;               /* 256 (== prompt / decoder width)                       */
    int32_t max_images;              /* encoder batch == number of embedding slots            */
    int32_t max_prompts;             /* prompts (boxes) of one samrs_predict pass; the decoder
                                        workspaces hold this many unless option "decode_prompts"
                                        raises it                                             */
    int32_t max_points;              /* max points per prompt                                 */
    int32_t precision;               /* enum samrs_precision                                  */
} samrs_config;

typedef struct samrs_engine samrs_engine_t;

/* -- lifetime ------------------------------------------------------------------------------
 * replaces: sam_model_registry[...](checkpoint) + sam.to(device) + SamPredictor(sam)
 * (main_sam_hbox_semantic.py:87-89).  `device` is the HIP device ordinal.  Returns NULL on
 * failure and writes a message into err (if non-NULL). */
samrs_engine_t* samrs_create(const samrs_config* cfg, int device, char* err, int err_len);
void samrs_destroy(samrs_engine_t* e);
const char* samrs_last_error(const samrs_engine_t* e);
int samrs_abi_version(void);

/* -- weights -------------------------------------------------------------------------------
 * replaces: sam.load_state_dict(state_dict) (build_sam.py:103-106).  One call per tensor with
 * the reference's key name, fp32, contiguous, HOST memory.  The engine
 * repacks into its MFMA operand layouts.  samrs_finalize_weights() fails with
 * SAMRS_ERR_BAD_WEIGHTS if any tensor is missing (strict). */
int samrs_load_weight(samrs_engine_t* e, const char* name, const float* host_data,
                      const int64_t* shape, int ndim);
int samrs_finalize_weights(samrs_engine_t* e, void* stream);

/* -- image side ----------------------------------------------------------------------------
 * replaces: SamPredictor.set_image / set_torch_image (predictor.py:34-90) incl.
 * Sam.preprocess (modeling/sam.py:164-174) and ImageEncoderViT.forward
 * (modeling/image_encoder.py:106-116).
 * `images`: n_images contiguous uint8 HWC RGB tiles of identical size in_h x in_w, ALREADY
 * resized so that max(in_h, in_w) == img_size (ResizeLongestSide.apply_image,
 * utils/transforms.py:26-31, stays on the host).  Embeddings land in slots
 * slot0 .. slot0+n_images-1. */
int samrs_set_images(samrs_engine_t* e, const uint8_t* images, int n_images, int in_h, int in_w,
                     int slot0, void* stream);
/* Ragged batch (the per-image H[] / W[] form): images[i] is the DEVICE pointer of tile i, in_h[i] x in_w[i]
 * with max(in_h[i], in_w[i]) == img_size; the three arrays themselves are HOST arrays of n_images
 * entries.  One encoder pass for tiles of different sizes (HRSC2016 / DIOR images after
 * ResizeLongestSide.apply_image, main_sam_rbox_mask_instance.py:99-101,157); each tile's embedding is
 * bit-identical to encoding it alone.  Remember each tile's (in_h, in_w) for samrs_predict. */
int samrs_set_images_ragged(samrs_engine_t* e, const uint8_t* const* images, const int* in_h,
                            const int* in_w, int n_images, int slot0, void* stream);
/* SamPredictor.get_image_embedding (predictor.py:247-258): fp32 [out_chans, 64, 64] (NCHW). */
int samrs_get_embedding(samrs_engine_t* e, int slot, float* out_chw, void* stream);
/* Install a precomputed embedding (fp32 NCHW) into a slot; marks it set. */
int samrs_set_embedding(samrs_engine_t* e, int slot, const float* emb_chw, void* stream);
/* SamPredictor.reset_image (predictor.py:264-271). */
int samrs_reset_image(samrs_engine_t* e, int slot);
/* The operand-split mode travels with the embedding (ABI 3): *split = the "split" option in force when the slot's image was
 * encoded (-1: installed by samrs_set_embedding), *split_depth = the number of leading blocks its block-GEMM bits covered.
 * samrs_predict(multimask = 1) on a slot whose mask lacks the block-GEMM bits this model's multimask outputs need (ViT-H: 64 or
 * 16; read-only option "grade_multimask") returns SAMRS_ERR_PRECISION instead of answering in whatever mode a single-mask
 * pipeline left behind -- unless option "allow_reduced" is 1 (set by an explicit SAMRS_SPLIT, or by the caller).  The
 * reference's SamPredictor.predict defaults to multimask_output=True (predictor.py:92-100, mask_decoder.py:101-106). */
int samrs_get_slot_info(const samrs_engine_t* e, int slot, int32_t* is_set, int32_t* split, int32_t* split_depth);

/* -- prompt side ---------------------------------------------------------------------------
 * replaces: SamPredictor.predict_torch (predictor.py:168-245) = PromptEncoder.forward
 * (modeling/prompt_encoder.py:128-173) + MaskDecoder.forward (modeling/mask_decoder.py:71-174)
 * + Sam.postprocess_masks (modeling/sam.py:133-162) + `> mask_threshold` (predictor.py:242-243).
 *
 *  boxes        [n_prompts,4] fp32 xyxy in the INPUT frame (after apply_boxes_torch) or NULL
 *  point_coords [n_prompts,n_points,2] fp32 input frame, or NULL
 *  point_labels [n_prompts,n_points] int32 (1 fg, 0 bg, -1 pad), required iff point_coords
 *  mask_input   [n_prompts,1,256,256] fp32 or NULL
 *  multimask    0 -> C = 1 (mask token 0), 1 -> C = 3 (tokens 1..3) (mask_decoder.py:102-107)
 *  return_logits 0 -> masks_out is uint8 {0,1} [n_prompts,C,orig_h,orig_w];
 *                1 -> masks_out is fp32 logits of the same shape
 *  in_h,in_w    size of the image handed to samrs_set_images (predictor.input_size)
 *  orig_h,orig_w size of the original image (predictor.original_size)
 *  masks_out / iou_out [n_prompts,C] / lowres_out [n_prompts,C,256,256]: caller-owned device
 *  buffers; any of them may be NULL to skip that output.
 *  n_prompts is unbounded like the reference's batch dimension: calls larger than the handle's
 *  max_prompts run as consecutive chunks on `stream` (results do not depend on the chunking).
 *  n_points is bounded by max_points (<= 8: the decoder keeps at most 16 tokens per prompt). */
int samrs_predict(samrs_engine_t* e, int slot, int n_prompts,
                  const float* boxes, const float* point_coords, const int32_t* point_labels,
                  int n_points, const float* mask_input, int multimask, int return_logits,
                  int in_h, int in_w, int orig_h, int orig_w,
                  void* masks_out, float* iou_out, float* lowres_out, void* stream);

/* Several images' prompts in one decoder chain (same outputs as one samrs_predict per image, fewer launches).
 *  n_images       >= 1; slots, prompt_offsets, in_hw, orig_hw and masks_out are HOST arrays read before the call returns
 *  slots          [n_images] embedding slots, all set; they may repeat and come in any order
 *  prompt_offsets [n_images + 1], prompt_offsets[0] = 0, non-decreasing: image i's prompts are rows
 *                 [prompt_offsets[i], prompt_offsets[i + 1]) of boxes / point_coords / point_labels / mask_input (the
 *                 layouts of samrs_predict); an image may have none.  The prompt kind (which arrays are present, n_points)
 *                 is the same for every image of a call.
 *  in_hw, orig_hw [n_images][2] input / original size (h, w) of each image
 *  masks_out      [n_images] device pointers, each [n_i, C, orig_h_i, orig_w_i] (uint8, or fp32 with return_logits), or
 *                 NULL (the array or an entry) to skip
 *  iou_out [total, C] / lowres_out [total, C, 256, 256]: contiguous over all prompts of the call, or NULL
 * Validation is that of samrs_predict for every image (SAMRS_ERR_NOT_SET names the slot; the multimask grade is checked per
 * slot).  One chain holds option "decode_prompts" prompts (default: max_prompts); larger calls run as consecutive chunks of that
 * size that may cross image boundaries; every output byte equals what samrs_predict(slots[i], ...) gives for image i alone. */
int samrs_predict_multi(samrs_engine_t* e, int n_images, const int* slots, const int* prompt_offsets,
                        const float* boxes, const float* point_coords, const int32_t* point_labels, int n_points,
                        const float* mask_input, int multimask, int return_logits,
                        const int* in_hw, const int* orig_hw, void* const* masks_out, float* iou_out, float* lowres_out,
                        void* stream);

/* -- "next row" N1: ordered painting + areas + class statistics on device --------------------
 * replaces the host loop of main_sam_hbox_semantic.py:195-206 and the sums of
 * statistic.py:15-21.  masks: uint8 [n,orig_h,orig_w] (the C = 1 output of samrs_predict),
 * labels: int32 [n] on device.  seg_mask (uint8 [orig_h,orig_w], caller initialises to 255,
 * :162) is overwritten in box order (later box wins).  areas_out int64 [n] = pixels per mask.
 * class_pixels / class_instances int64 [n_classes] are ACCUMULATED (area > 0 only); either may
 * be NULL. */
int samrs_paint(samrs_engine_t* e, const uint8_t* masks, const int32_t* labels, int n,
                int orig_h, int orig_w, uint8_t* seg_mask, int64_t* areas_out,
                int64_t* class_pixels, int64_t* class_instances, int n_classes, void* stream);

/* -- BASELINE.json configs[3] (the rbox / rhbox instance path WITH multimask_output=True; the reference's own scripts,
 * main_sam_rhbox_mask_instance.py:168 / main_sam_rbox_mask_instance.py:164 / main_sam_hbox_mask_instance.py:165, all pass
 * multimask_output=False and need none of this): of the n_sel masks per object keep the one with the highest predicted IoU (first maximum),
 * replacing the host-side `argmax` / gather / `.sum()`.  masks uint8 [n][n_sel][h][w], iou fp32 [n][n_sel] (both outputs of
 * samrs_predict) -> best_out uint8 [n][h][w], quality_out fp32 [n], areas_out int64 [n] (pixels set). */
int samrs_select_best(samrs_engine_t* e, const uint8_t* masks, const float* iou, int n, int n_sel, int h, int w,
                      uint8_t* best_out, float* quality_out, int64_t* areas_out, void* stream);

/* -- HRSC instance evaluation (main_sam_rhbox_mask_instance.py:204-214, :222-238).
 * masks uint8 [n][h][w] (non-zero = set; the kept masks of samrs_select_best), label_rgb uint8 [h][w][3],
 * colors uint8 [n][3], all on the device.  Instance j's ground truth = the pixels whose RGB equals colors[j].
 * inter_out[j] = |mask_j AND gt_j|, gt_area_out[j] = |gt_j| (int64, overwritten).  gt_masks_out uint8 [n][h][w] (0/1) or NULL.
 * The union is pred_area + gt_area - inter with pred_area from samrs_select_best; gt_masks_out is what samrs_rle_encode takes
 * for the ground truth's COCO RLE.  The label image is read once per call, not once per instance.  h * w < 2^30. */
int samrs_gt_match(samrs_engine_t* e, const uint8_t* masks, int n, int h, int w, const uint8_t* label_rgb,
                   const uint8_t* colors, int64_t* inter_out, int64_t* gt_area_out, uint8_t* gt_masks_out, void* stream);

/* -- the reference's per-instance output: COCO RLE of every full-resolution mask (main_sam_hbox_semantic.py:201-202:
 * `maskUtils.encode(np.asfortranarray(mask))` + `.decode('ascii')`; counts half stated in-tree at utils/amg.py:107-135).
 * masks: uint8 [n][h][w] on device (non-zero = set; the C = 1 output of samrs_predict).  The n ASCII strings are packed into
 * `out` (device bytes, capacity out_capacity) at 16-byte aligned offsets behind *cursor (device int64, in / out: the first
 * free byte; several calls append to one buffer), and table [n][3] (device int64) receives (offset, length, number of counts)
 * per mask; length < 0 means the string did not fit (-length - 1 bytes were needed) and was not written.  Column-major runs
 * starting with zeros, delta-coded 5-bit groups + 48, exactly as cocoapi's rleToString.  h * w < 2^30, w <= 8192.
 * The run table this entry point builds lives in ONE scratch buffer per handle: all samrs_rle_encode calls on a handle must be
 * stream-ordered with each other (same stream, or an event between them); two handles never share it. */
int samrs_rle_encode(samrs_engine_t* e, const uint8_t* masks, int n, int h, int w, uint8_t* out, int64_t out_capacity,
                     int64_t* cursor, int64_t* table, void* stream);

/* -- scene mode: a scene larger than the encoder's input is decoded window by window (samrs_amd/scene.py plans the windows; every
 * box is decoded in exactly one), and the windows' masks are composited in the scene's own frame on the device.  The reference's
 * rule "boxes are painted in annotation order, a later box wins" (main_sam_hbox_semantic.py:162,195-199) holds across windows
 * through a caller-owned map of the highest annotation rank set at each pixel.
 *
 * samrs_scene_claim: masks uint8 [n][h][w] (non-zero = set): the masks of one predict call, all decoded in the window
 * (x0, y0, w, h) of an H x W scene.  ranks int32 [n] (device): each mask's position in the scene's annotation order.  order int32
 * [H][W], caller-owned, initialised to -1: order[p] = max(order[p], max{ranks[j] : mask j set at p}).  areas_out / class_pixels /
 * class_instances: exactly samrs_paint's (labels int32 [n], may be NULL when both class arrays are).  A pixel has one writer per
 * call: calls on one map must be stream-ordered with each other, and then the map does not depend on their order.  n == 0 is a
 * no-op.  16-byte mask loads when w % 16 == 0 and masks is 16-byte aligned, byte loads otherwise.
 * samrs_scene_resolve: seg[p] = order[p] < 0 ? 255 : (uint8) labels_by_rank[order[p]] (labels_by_rank int32 [n_ranks], device; a
 * rank >= n_ranks resolves to 255).
 * A window not inside the scene, n < 0 or a null pointer: SAMRS_ERR_BAD_ARG, and nothing is written. */
int samrs_scene_claim(samrs_engine_t* e, const uint8_t* masks, const int32_t* ranks, const int32_t* labels, int n, int h, int w,
                      int x0, int y0, int H, int W, int32_t* order, int64_t* areas_out,
                      int64_t* class_pixels, int64_t* class_instances, int n_classes, void* stream);
int samrs_scene_resolve(samrs_engine_t* e, const int32_t* order, const int32_t* labels_by_rank, int n_ranks, int H, int W,
                        uint8_t* seg, void* stream);
/* samrs_rle_encode of each mask as if pasted at (x0, y0) on an all-zero H x W canvas, without materialising the canvas: table /
 * cursor / overflow protocol unchanged; the strings are those of {"size": [H, W]}.  H * W < 2^30 and w < 8192; a window not inside
 * the canvas, n < 0 or a size over the limit: SAMRS_ERR_BAD_ARG.  n == 0 is a no-op.  Shares the handle's RLE scratch with
 * samrs_rle_encode (stream-ordered with each other); a call with many or large masks runs as consecutive chunks on the stream so
 * that the scratch stays below 256 MiB, or one mask's worth. */
int samrs_rle_encode_placed(samrs_engine_t* e, const uint8_t* masks, int n, int h, int w, int x0, int y0, int H, int W,
                            uint8_t* out, int64_t out_capacity, int64_t* cursor, int64_t* table, void* stream);

/* -- the inverse of samrs_rle_encode: COCO RLE strings -> masks, on the device.  strings: device bytes [strings_bytes]; table [n][3]
 * (device int64) has exactly the layout samrs_rle_encode writes, (offset, length, n_counts), n_counts ignored on input: an encode
 * call's `out` + `table` can be fed straight back.  Offsets need no alignment.  masks_out uint8 [n][h][w], row-major 0 / 1, every
 * byte of it written; areas_out [n] (device int64, or NULL) = set pixels of mask j; status_out [n] (device int32) = the
 * lowest-numbered samrs_rle_status that applies.  A mask with a non-zero status is all zero and has area 0.  The format is cocoapi's
 * rleFrString: char - 48, 5-bit groups, bit 5 = continuation, bit 4 of the last group sign-extends, from the 4th count on a delta
 * against the count two back; counts are column-major runs starting with zeros, and zero-length counts are legal anywhere.
 * The strings are untrusted: a mask is filled only after its whole string validated, sums are taken in 64 bits, no index derived
 * from string bytes reaches memory unchecked, and the call is memory-safe for arbitrary bytes and table rows.  A delta that does not
 * fit int32 is taken as saturated (its count is negative or above 2^30 either way).  The table rows of a call name distinct strings:
 * a row that brings the summed lengths of its chunk of the call (up to 32 masks) above strings_bytes is reported RANGE.
 * h * w < 2^30, h, w >= 1, strings_bytes < 2^31.  n == 0 is a no-op; a null handle or pointer, n < 0 or a size over the limit:
 * SAMRS_ERR_BAD_ARG and nothing is launched.  Integer arithmetic only: bit-exact with samrs_amd/rle.py:decode.
 * The token / count / boundary arrays (4 bytes per byte of `strings`) and the bit matrix live in ONE scratch buffer per handle, its
 * own: all samrs_rle_decode calls on a handle must be stream-ordered with each other (same stream, or an event between them); two
 * handles never share it.  A call with many or large masks runs as consecutive chunks on the stream (32 masks or 64 MiB of bit matrix
 * at most, one mask at least). */
enum samrs_rle_status {
    SAMRS_RLE_OK = 0,          /* the mask was decoded                                             */
    SAMRS_RLE_ABSENT = 1,      /* length < 0: the encoder's "did not fit" marker                   */
    SAMRS_RLE_RANGE = 2,       /* offset < 0 or offset + length > strings_bytes                    */
    SAMRS_RLE_BAD_CHAR = 3,    /* a byte outside 48..111                                           */
    SAMRS_RLE_TRUNCATED = 4,   /* the last char has the continuation bit                           */
    SAMRS_RLE_BAD_COUNT = 5,   /* a token of more than 7 chars, or a count negative after the delta */
    SAMRS_RLE_BAD_SUM = 6      /* the counts do not sum to exactly h * w (the empty string too)    */
};
int samrs_rle_decode(samrs_engine_t* e, const uint8_t* strings, int64_t strings_bytes, const int64_t* table, int n, int h, int w,
                     uint8_t* masks_out, int64_t* areas_out, int32_t* status_out, void* stream);

/* -- mask clean-up before the masks become labels: `remove_small_regions` of utils/amg.py:267-291 on the device, for a batch of
 * masks that never leave HBM (the reference's runs on the host through cv2, one mask per call).  masks uint8 [n][h][w] device, in /
 * out (non-zero = set in, 0 / 1 out): the C = 1 output of samrs_predict, or the kept masks of samrs_select_best.  A region is an
 * 8-connected component; it is small when it has fewer than min_area pixels (a region of exactly min_area pixels stays).
 *   SAMRS_REGION_HOLES    every unset pixel in a small component of the complement becomes set;
 *   SAMRS_REGION_ISLANDS  every set pixel in a small component is cleared; if EVERY component is small, exactly one is kept, the
 *                         largest (amg.py:287-289) -- among equally large ones the one whose first pixel in row-major order comes
 *                         first.  That tie rule is this library's: the reference takes np.argmax over cv2's label numbers, whose
 *                         order cv2 does not promise;
 *   SAMRS_REGION_BOTH     holes, then islands on the result (automatic_mask_generator.py postprocess_small_regions).
 * areas_out int64 [n] = pixels set after the cleanup, changed_out int64 [n] = pixels whose value changed (either may be NULL).
 * Integer arithmetic only, bitwise reproducible, no host synchronisation; h * w < 2^30, any h, w >= 1.  Labels and areas (8 bytes
 * per pixel per mask in flight; a call with more than 32 masks runs as consecutive chunks of 32 on the stream: 256 MiB at 1024^2)
 * live in ONE scratch buffer per handle that grows on demand: all samrs_clean_masks calls on a handle must be stream-ordered with
 * each other (same stream, or an event between them); two handles never share it. */
enum samrs_region_mode { SAMRS_REGION_HOLES = 1, SAMRS_REGION_ISLANDS = 2, SAMRS_REGION_BOTH = 3 };
int samrs_clean_masks(samrs_engine_t* e, uint8_t* masks, int n, int h, int w, int min_area, int mode,
                      int64_t* areas_out, int64_t* changed_out, void* stream);

/* -- where a mask actually is: the tight horizontal box and the minimum-area rotated box of every mask, derived on the device from
 * the masks themselves (the `bbox` the reference stores is the PROMPT box; its oriented annotations -- DOTA text form, `Generate
 * Dataset/ann_transform.py:46` -- come from cv2.findContours + cv2.minAreaRect on the host).  masks uint8 [n][h][w] device (non-zero
 * = set), decoded in a window whose origin is (x0, y0) in the frame the boxes are wanted in.
 *   points      the set pixels as integer points (x0 + col, y0 + row): pixel CENTRES, cv2's convention;
 *   hbox_out    int32 [n][4] = xmin, ymin, xmax, ymax, inclusive;
 *   hull        the strict vertices of the convex hull (no collinear points), from v0 = the set pixel with the smallest (y, x), down
 *               the left side, along the last non-empty row, up the right side, back to v0; m vertices (1 for one pixel, 2 for
 *               collinear pixels);
 *   candidates  edge k = vertex k -> vertex (k + 1) mod m with (dx, dy) their difference (not reduced); over the hull vertices
 *               p = x dx + y dy, q = -x dy + y dx; area (pmax - pmin)(qmax - qmin) / (dx^2 + dy^2), an exact rational;
 *   winner      the smallest area, compared exactly; ties go to the smallest k (this library's rule).  m = 1: (dx, dy) = (1, 0);
 *   rbox_out    fp32 [n][4][2]: the corners (pmin, qmin), (pmax, qmin), (pmax, qmax), (pmin, qmax) as x = (p dx - q dy) / L,
 *               y = (p dy + q dx) / L, L = dx^2 + dy^2: an exact integer numerator, one correctly rounded fp64 division, rounded
 *               to fp32;
 *   record_out  int64 [n][8]: dx, dy, pmin, pmax, qmin, qmax, m, twice the hull's area (shoelace sum over the ordered vertices):
 *               convexity = mask area / hull area comes for free.
 * An empty mask has m = 0 and all its outputs zero.  Any output may be NULL.  Not pinned against cv2 itself: cv2.minAreaRect works
 * from the same hull, so it can differ only in float rounding and in which of several equal-area rectangles it returns.
 * h, w <= 8192, x0, y0 >= 0, x0 + w <= 32768 and y0 + h <= 32768; outside these limits, n < 0 or masks == NULL:
 * SAMRS_ERR_BAD_ARG and nothing is written.  n == 0 is a no-op.  Integer arithmetic up to the one division per coordinate,
 * bitwise reproducible, no host synchronisation.  The row extents (12 bytes per mask row; a call whose extents would exceed 64 MiB
 * runs as consecutive chunks on the stream) live in ONE scratch buffer per handle that grows on demand: all samrs_mask_boxes calls
 * on a handle must be stream-ordered with each other (same stream, or an event between them); two handles never share it. */
int samrs_mask_boxes(samrs_engine_t* e, const uint8_t* masks, int n, int h, int w, int x0, int y0,
                     int32_t* hbox_out /*[n][4]*/, float* rbox_out /*[n][4][2]*/, int64_t* record_out /*[n][8]*/, void* stream);

/* -- a mask's outline as polygons: outer rings and holes of every mask, traced on the device (annotation tools, iSAID-style
 * instance files and DOTA-style oriented annotations consume polygons; the reference goes through cv2.findContours on the host, one
 * mask at a time).  masks uint8 [n][h][w] device (non-zero = set; outside the image counts as unset), decoded in a window whose
 * origin is (x0, y0).  All geometry is on the pixel LATTICE: vertex (x, y), 0 <= x <= w, 0 <= y <= h, is the top-left CORNER of pixel
 * (row y, col x) -- deliberately NOT the pixel centres of samrs_mask_boxes: the polygon encloses exactly the set pixels' squares.
 *   crack edge  a unit lattice segment between a set pixel and an unset one, directed so that the set pixel is on the right hand of
 *               travel (y down).  Set pixel p = y w + x owns id = 4 p + d: d = 0 top, (x, y) -> (x + 1, y); 1 right, (x + 1, y) ->
 *               (x + 1, y + 1); 2 bottom, (x + 1, y + 1) -> (x, y + 1); 3 left, (x, y + 1) -> (x, y);
 *   successor   at the end vertex of pixel P's edge d, with R the pixel straight ahead of P and L the pixel ahead on the left: L set:
 *               L's edge (d + 3) % 4 (a saddle vertex joins the diagonal pixels: the foreground is 8-connected, the regions of
 *               samrs_clean_masks); else R set: R's edge d; else P's own edge (d + 1) % 4.  A bijection: the edges fall into rings;
 *   ring        ranked from its smallest edge id (a top edge for an outer ring, a bottom edge for a hole) along the successor; an
 *               edge is a corner when its direction differs from its predecessor's; the polygon is the start vertices of the corner
 *               edges in rank order (collinear lattice points dropped, no other simplification; a hole's polygon starts at the first
 *               corner behind its rank-0 edge; a ring may touch itself at a saddle vertex).  Outer rings run clockwise on screen;
 *   order       the rings of a mask by ascending smallest edge id, masks in call order;
 *   vertices    int32 [vertex_capacity][2] = (x0 + x, y0 + y);
 *   rings       int32 [ring_capacity][4] = first vertex relative to the mask's first vertex, vertex count, twice the signed area
 *               (shoelace; > 0 outer ring, < 0 hole; over a mask's rings it sums to twice the set pixels), the pixel index y w + x
 *               of the ring's smallest edge (a set pixel of the ring's component);
 *   table       int64 [n][5] = first ring, ring count, first vertex, vertex count, edge count; the firsts are absolute indices into
 *               the two buffers; an empty mask has counts 0;
 *   cursor      int64 [2] device, in / out: first free vertex, first free ring.  Masks are placed in order behind it, so several
 *               calls append to one pair of buffers (as samrs_rle_encode does with its buffer).
 * A mask that does not fit either capacity is skipped and takes no space: first ring = first vertex = -1, ring count = -1 - rings
 * needed, vertex count = -1 - vertices needed; later masks are still placed if they fit.  A mask with edge count > max_edges is not
 * traced: ring count = vertex count = -1, firsts -1; edge count is always the true number.  max_edges bounds the scratch (about 73
 * bytes per edge and mask in flight) and the ceil(log2(min(max_edges, 4 h w))) ranking rounds (pointer doubling on the cycles).
 * h, w, x0, y0 within samrs_mask_boxes's limits and h * w < 2^30; outside them, n < 0, max_edges < 4 or a null masks / vertices /
 * rings / cursor / table: SAMRS_ERR_BAD_ARG and nothing is written.  n == 0 is a no-op.  Integer arithmetic only, bitwise
 * reproducible, no host synchronisation.  ONE scratch buffer per handle grows on demand (a big call runs as consecutive chunks on the
 * stream so that it stays at or below 256 MiB, or one mask's worth): all samrs_mask_polygons calls on a handle must be stream-ordered
 * with each other; two handles never share it. */
int samrs_mask_polygons(samrs_engine_t* e, const uint8_t* masks, int n, int h, int w, int x0, int y0, int max_edges,
                        int32_t* vertices /* [vertex_capacity][2] */, int64_t vertex_capacity,
                        int32_t* rings /* [ring_capacity][4] */, int64_t ring_capacity,
                        int64_t* cursor /* device [2], in / out: first free vertex, first free ring */,
                        int64_t* table /* device [n][5] */, void* stream);

/* -- the traced rings simplified in place: Douglas-Peucker on every closed ring, distances to the chord SEGMENT, integers only (what
 * polygon consumers otherwise do with cv2.approxPolyDP / shapely's simplify on the host, one ring at a time).  The rule, which is the
 * definition (tests/polygon_simplify_ref.py restates it as a plain recursion over Python ints):
 *   tolerance   eps_q, in sixteenths of a pixel, 1 <= eps_q <= 16384;
 *   frame       a ring has the vertices v[0 .. k - 1] (k >= 4 for a lattice ring) in the order samrs_mask_polygons wrote.  Only
 *               coordinate differences enter, so the offset (x0, y0) cannot matter.  Within samrs_mask_boxes's limits (h, w <= 8192)
 *               a difference is at most 2^13 in magnitude, a squared length or a cross / dot product at most 2^27, and every product
 *               below (N <= 2^54, 256 N <= 2^62, eps_q^2 D <= 2^55) fits in int64;
 *   anchors     always kept: A = index 0; B = the index with the greatest |v[i] - v[A]|^2; C = the index with the greatest
 *               |cross(v[B] - v[A], v[i] - v[A])|; ties go to the smallest index.  A traced ring has non-zero area, so C has a
 *               non-zero cross product: every ring keeps at least 3 vertices that are not collinear.  The anchors in index order
 *               cut the ring into three chains; the last one closes on index 0 again;
 *   chain (i, j)  both ends are kept; a = v[i], b = v[j], L = |b - a|^2.  Every interior vertex p = v[m] has the numerator N(m) of its
 *               squared distance to the segment over the common denominator D: L == 0 (one lattice point visited twice, at a saddle
 *               vertex): N = |p - a|^2, D = 1; otherwise D = L and, with t = dot(p - a, b - a): t <= 0: N = |p - a|^2 L; t >= L:
 *               N = |p - b|^2 L; else N = cross(b - a, p - a)^2.  m* = the interior vertex with the greatest N, ties to the smallest
 *               m.  If N(m*) > floor(eps_q^2 D / 256) (that is 256 N > eps_q^2 D), m* is kept and (i, m*), (m*, j) are treated the
 *               same way; otherwise every interior vertex is dropped.  The result depends on the ring and eps_q only, not on the
 *               order in which chains are processed;
 *   result      the kept vertices in index order, starting with v[0].
 * Topology is NOT preserved (a simplified ring may touch or cross itself or a neighbour; so may approxPolyDP's), and the rule is not
 * pinned against cv2.
 * The call works IN PLACE on what consecutive samrs_mask_polygons calls of this handle wrote behind one cursor: table int64 [n][5] holds
 * the n rows of those calls in placement order, whose placed masks cover the vertices [v0, cursor[0]) contiguously, v0 = the first
 * vertex of the first placed row.  The vertices of that range are compacted towards v0 in order; each ring record's first vertex
 * (relative to its mask's) and vertex count, and each placed row's first vertex and vertex count, are rewritten; cursor[0] becomes the
 * new end (it stays as it is when no row is placed).  Unchanged: ring positions and counts, cursor[1], the table's edge count, a ring
 * record's pixel index, and its third field, which stays the ORIGINAL ring's twice-signed area -- hole or outer is still its sign, a
 * mask's rings still sum to twice its set pixels, and the simplified ring's own area is one shoelace sum away.  Rows with negative
 * counts (not traced, not placed) pass through untouched; an empty mask keeps its zero counts.  n == 0 is a no-op.  A null handle /
 * vertices / rings / table / cursor, n < 0, eps_q outside 1 .. 16384, or buffers into which this handle has not traced (the handle
 * remembers the capacities samrs_mask_polygons was given for them; that is what bounds the scratch without reading the cursor back):
 * SAMRS_ERR_BAD_ARG and nothing is written.  Integer arithmetic only, bitwise reproducible, no host synchronisation.  Keep flags,
 * per-ring counts, their scan and the staging copy of the compaction (21 bytes per vertex and 36 per ring of the capacities, 8 per row) live in
 * samrs_mask_polygons's scratch buffer: the call must be stream-ordered with every samrs_mask_polygons / samrs_simplify_polygons call
 * on the handle. */
int samrs_simplify_polygons(samrs_engine_t* e, int32_t* vertices, int32_t* rings, int64_t* table /* device [n][5] */, int n, int eps_q,
                            int64_t* cursor /* device [2] */, void* stream);

/* -- rings back to masks: the even-odd fill of the rings of n table rows, sampled at the pixel centres, integers only -- the inverse of
 * samrs_mask_polygons, and the raster that belongs to rings samrs_simplify_polygons or a caller has changed (what polygon consumers
 * otherwise do on the host edge by edge: samrs_amd/polygons.py rasterize_any, cv2.fillPoly).  vertices / rings / table are exactly
 * what samrs_mask_polygons writes and samrs_simplify_polygons rewrites: table int64 [n][5] with absolute first ring and first vertex,
 * ring records whose first field is the ring's first vertex relative to its mask's and whose second is its vertex count; a ring
 * record's area and pixel-index fields and the table's edge count are NOT read, so a caller may build the three arrays on the host
 * from any integer polygons (samrs_amd/polygons.py pack_rings).  The rule, which is the definition (tests/polygon_fill_ref.py restates
 * it as a per-pixel crossing count over Python ints):
 *   frame     (x0, y0) is subtracted from every vertex; pixel (r, c), 0 <= r < h, 0 <= c < w, has its centre at (c + 1/2, r + 1/2).
 *             A vertex farther than 2^20 from (x0, y0) in either coordinate makes its row "not rings" (below): within that bound a
 *             coordinate difference is at most 2^21 in magnitude and every product below stays under 2^45, far inside int64;
 *   edges     (xa, ya) -> (xb, yb), consecutive vertices of a ring; the ring's last vertex closes on its first.  Horizontal edges
 *             (ya == yb) never count.  An edge acts on the rows r with min(ya, yb) <= r < max(ya, yb): those whose centre line it
 *             crosses -- the vertices are integers, so a centre line never passes through a vertex;
 *   toggle    in such a row the edge crosses the centre line at X = xa + (xb - xa) (2 r + 1 - 2 ya) / (2 (yb - ya)) and toggles every
 *             pixel c whose centre is at or right of it, c + 1/2 >= X: a centre exactly on an edge counts as right of it.  With the
 *             edge oriented so that dy = yb - ya > 0 and dx = xb - xa, the first toggled column is
 *             ceil(((2 xa - 1) dy + dx (2 r + 1 - 2 ya)) / (2 dy)), clamped to [0, w] (w: the edge toggles nothing in that row);
 *   pixel     (r, c) is 1 iff an odd number of the edges of ALL rings of the row toggle it, 0 otherwise (even-odd): holes, islands
 *             inside holes, rings that cross themselves or each other all follow from that.
 * masks_out [n][h][w] (or NULL): every byte written, 0 / 1.  counts_out int64 [n][3] (or NULL): (set pixels of the fill, set pixels of
 * ref[j] -- non-zero bytes --, pixels set in both); without ref the last two are 0.  It is zeroed by the call itself, on the stream.
 * With masks_out NULL only the counts are taken and nothing of size h * w is written; both NULL: SAMRS_ERR_BAD_ARG.
 * Rows that are not rings: a negative ring or vertex count (not traced / not placed), a vertex beyond the 2^20 bound, counts of 2^30 or
 * more, negative firsts, vertices without rings, or ring records that do not tile the row's vertex range in order (the first begins
 * at 0, each begins where its predecessor ends, none is empty, the last ends at the vertex count) fill as the empty mask and report
 * counts[j][0] = -1; ref[j] is still counted.  A row with zero rings (and zero vertices) is the empty mask: (0, ref area, 0).  The
 * table and the ring records are treated as untrusted in that sense, but the capacities are not arguments: a row's firsts and counts
 * are believed to lie inside the buffers.  No store leaves [n][h][w] / [n][3].
 * h, w, x0, y0 within samrs_mask_boxes's limits (h, w in 1..8192, x0, y0 >= 0, x0 + w, y0 + h <= 32768).  n == 0 is a no-op; a null
 * handle / vertices / rings / table, n < 0, a shape outside the limits: SAMRS_ERR_BAD_ARG and nothing is written.  One kernel, the
 * band's bits in LDS: no scratch buffer, so no stream-ordering rule beyond the caller's own for its buffers.  Integer arithmetic only,
 * bitwise reproducible, no host synchronisation. */
int samrs_fill_polygons(samrs_engine_t* e, const int32_t* vertices, const int32_t* rings, const int64_t* table /* device [n][5] */,
                        int n, int h, int w, int x0, int y0,
                        uint8_t* masks_out /* device [n][h][w] or NULL */, const uint8_t* ref /* device [n][h][w] or NULL */,
                        int64_t* counts_out /* device [n][3] or NULL */, void* stream);

/* -- mask quality before the masks become labels: the three signals a box-prompted mask carries, counted on the device straight
 * from the 256^2 logits (`calculate_stability_score`, utils/amg.py:156-176, and the `pred_iou_thresh` / `stability_score_thresh`
 * gate of automatic_mask_generator.py:295-304; the box fit is this library's own).  lowres fp32 [n][256][256]: the lowres_out of
 * samrs_predict with C flattened into n (for C = 3 the caller repeats the boxes).  v(p) = the value samrs_predict's postprocess
 * computes at output pixel p for (in_h, in_w, orig_h, orig_w) -- the very same arithmetic, so the second count equals the number of
 * set bytes of the uint8 mask samrs_predict writes for the same logits, exactly.  counts_out int64 [n][4], overwritten:
 *   n_hi  = #{v > +offset}      n_mid = #{v > 0} (SAM's mask_threshold)      n_lo = #{v > -offset}
 *   n_in  = #{v > 0 and bx0 <= (float)x <= bx1 and by0 <= (float)y <= by1}: boxes fp32 [n][4] xyxy in the ORIGINAL frame, or
 *           NULL (n_in = 0).
 * stability = n_hi / n_lo, share inside the box = n_in / n_mid.  The full-resolution logits are never materialised: 256 KiB read
 * and 32 bytes written per mask.  offset >= 0 and finite (0: three equal counts); orig_h * orig_w < 2^31; in_h, in_w <= img_size
 * with max(in_h, in_w) == img_size.  n < 0, a null lowres / counts_out, a bad offset or size: SAMRS_ERR_BAD_ARG and nothing is
 * written.  n == 0 is a no-op.  Integer atomics only: bitwise reproducible; no host synchronisation, no scratch on the handle. */
int samrs_score_masks(samrs_engine_t* e, const float* lowres, int n, int in_h, int in_w, int orig_h, int orig_w,
                      float offset, const float* boxes /* [n][4] or NULL */, int64_t* counts_out /* [n][4] */, void* stream);
/* The gate itself: keep_out[j] = 1 iff every enabled criterion holds, else 0 and mask j (uint8 [n][h][w], in / out) is zeroed in
 * place; a kept mask is not touched.  A threshold <= 0 disables its criterion (amg.py:295,303).  Compared in fp64 from the fp32
 * arguments and the integer counts of samrs_score_masks (counts int64 [n][4]):
 *   stability      n_lo > 0 && (double)n_hi >= (double)min_stability * (double)n_lo   (>=, as the reference; an empty low-threshold
 *                  mask fails -- the reference's 0 / 0 is NaN, which fails too; that reading is this library's rule);
 *   predicted IoU  iou[j] > min_pred_iou   (strict, as the reference; iou fp32 [n], NULL with the criterion on: SAMRS_ERR_BAD_ARG);
 *   box fit        n_mid == 0 || (double)n_in >= (double)min_inside * (double)n_mid   (an empty mask passes: this library's rule).
 * A dropped mask is an empty mask to everything downstream: samrs_paint paints nothing and counts area 0 (no class statistics),
 * samrs_mask_boxes reports m = 0.  16-byte stores when masks is 16-byte aligned and h * w % 16 == 0, byte stores otherwise.
 * n < 0, h or w < 1, a null masks / counts / keep_out: SAMRS_ERR_BAD_ARG and nothing is written.  n == 0 is a no-op. */
int samrs_filter_masks(samrs_engine_t* e, uint8_t* masks, int n, int h, int w, const int64_t* counts /* [n][4] */,
                       const float* iou /* [n] or NULL */, float min_stability, float min_pred_iou, float min_inside,
                       uint8_t* keep_out /* [n] */, void* stream);

/* -- one instance per pixel: where several masks of a call are set at the same pixel, the pixel is given to exactly one of them and
 * cleared in the others, in place, so that everything downstream (samrs_paint, areas, class statistics, samrs_rle_encode,
 * samrs_mask_boxes, samrs_mask_polygons) sees disjoint masks.  Without this stage the only overlap rule is samrs_paint's painting
 * order -- a later box wins (main_sam_hbox_semantic.py:195-199) -- and it reaches the class map alone.
 * masks uint8 [n][h][w] device, in / out (non-zero = set); (h, w) = the original size the masks were decoded at.
 *   the rule  walk j = 0 .. n-1 and keep a holder per pixel.  Mask j is a candidate at p iff its byte is set.  It replaces holder b iff
 *             there is no holder, or P[j] > P[b], or P[j] == P[b] and not v_j(p) < v_b(p).  Ties and non-comparable values (NaN)
 *             therefore go to the LATER mask, as painting does.  P[j] is an int64 primary key per mask, v_j(p) the postprocessed
 *             logit of mask j at p: the value samrs_predict's postprocess computes there for (in_h, in_w, h, w) from lowres fp32
 *             [n][256][256] -- the very same arithmetic as samrs_score_masks, never materialised.  With lowres NULL the logit term is
 *             absent (treated as equal: the later mask of equal key wins).
 *   the gate  is the mask BYTE, not v > 0: a pixel that samrs_clean_masks filled competes, with its negative logit, and a pixel
 *             that samrs_filter_masks or the clean-up cleared does not.
 *   SAMRS_OVERLAP_LOGIT     P[j] = 0: the highest logit wins.  Needs lowres.
 *   SAMRS_OVERLAP_SMALLEST  P[j] = -(set pixels of mask j on entry): the smaller instance wins (a ship inside a harbour); equal areas
 *                           fall to the logit if lowres is given, then to the later mask.  The call counts the entry areas itself,
 *                           in a first launch.
 *   SAMRS_OVERLAP_PRIORITY  P[j] = priority[j], the caller's device int64 [n]; equal keys as above.
 * Every loser's byte is set to 0; a winner's byte is not touched (a 0/1 mask stays 0/1, a 0/255 mask 0/255).  Optional outputs, each
 * may be NULL: owner_out int32 [h][w] = index of the winner, -1 where no mask is set; before_out int64 [n] = set pixels on entry;
 * removed_out int64 [n] = pixels cleared (before - removed = set pixels afterwards).
 * (in_h, in_w): the input frame, in_h, in_w <= img_size with max(in_h, in_w) == img_size as samrs_score_masks; only read when
 * lowres is given.  n < 0, a null masks, an unknown rule, LOGIT without lowres, PRIORITY without priority, h or w < 1, a bad input
 * frame or h * w >= 2^31: SAMRS_ERR_BAD_ARG and nothing is written.  n == 0 is a no-op; n == 1 changes no mask and still fills the
 * outputs.  A pixel has one owning thread and the counts use integer atomics only: bitwise reproducible; no host synchronisation.
 * Cost: the n h w mask bytes are read once; only the threads with a contested pixel read them again and evaluate logits there.
 * Rule SMALLEST with before_out NULL keeps its 8 n bytes of entry areas in ONE scratch buffer per handle that grows on demand: such
 * calls on a handle must be stream-ordered with each other (same stream, or an event between them); two handles never share it.
 * Every other form uses no scratch. */
enum samrs_overlap_rule { SAMRS_OVERLAP_LOGIT = 1, SAMRS_OVERLAP_SMALLEST = 2, SAMRS_OVERLAP_PRIORITY = 3 };
int samrs_resolve_overlaps(samrs_engine_t* e, uint8_t* masks, int n, int h, int w, int rule,
                           const float* lowres /* [n][256][256] or NULL */, int in_h, int in_w,
                           const int64_t* priority /* [n], rule PRIORITY */,
                           int32_t* owner_out /* [h][w] or NULL */, int64_t* before_out /* [n] or NULL */,
                           int64_t* removed_out /* [n] or NULL */, void* stream);

/* -- COCO mask AP on the device: every prediction of an image against every ground truth of it (samrs_gt_match counts the diagonal
 * only), and COCOeval.evaluateImg's greedy matching.  The two JSON files of the instance drivers exist for this number
 * (main_sam_rhbox_mask_instance.py:246-255, "Obtain COCO format for AP calculation").
 * Bit planes: uint64 [n][words], words = ceil(h * w / 64); pixel p (row-major) is bit p % 64 of word p / 64, the unused high bits of
 * the last word are zero.  An eighth of the mask bytes, so a tile's planes can be kept while its masks are decoded chunk by chunk.
 *   samrs_mask_pack_bits   masks uint8 [n][h][w] (non-zero = set) -> planes_out.  Any alignment; 16-byte loads where h * w % 16 == 0
 *                          and masks is 16-byte aligned.
 *   samrs_label_pack_bits  the ground truth straight from label_rgb uint8 [h][w][3] and colors uint8 [n][3]: instance j = the pixels
 *                          whose RGB equals colors[j] (duplicate colours give equal planes, an absent colour an empty one).  The
 *                          label image is read once per call, not once per instance; no mask bytes are materialised.
 *   samrs_mask_pair_counts a uint64 [na][words], b uint64 [nb][words] -> inter_out int64 [na][nb] = popcount(a[i] & b[j]),
 *                          area_a_out int64 [na] / area_b_out int64 [nb] = popcount of each plane (each may be NULL).  Integer
 *                          atomics into outputs the call zeroes: exact and bitwise reproducible.  a == b is allowed.
 * All on the device, no host synchronisation, no scratch.  h * w < 2^30 (words <= 2^24).  A null handle or pointer, a negative count,
 * h, w or words < 1 or a size over the limit: SAMRS_ERR_BAD_ARG and nothing is launched.  n == 0 is a no-op; with na == 0 or nb == 0
 * there are no pairs and the areas of the other side are still counted.
 *
 * samrs_coco_match: the matching of one image and one category, for n_ranges area ranges x n_thresholds IoU thresholds at once.
 *   inputs   inter int64 [nd][ng], area_d int64 [nd], area_g int64 [ng] (the outputs of samrs_mask_pair_counts) and scores fp32 [nd]
 *            on the device; thresholds double [n_thresholds] and area_ranges double [n_ranges][2] = (lo, hi) on the HOST (read
 *            before the call returns).  scores_on_host != 0: scores is a host array; it is checked and copied to the device by
 *            the call and must stay unchanged until the stream has passed the call.
 *   order    detection d precedes e iff score[d] > score[e], or the scores are equal and d < e (a stable descending sort); the
 *            first max_det are kept: n_kept = min(nd, max_det).
 *   ignore   for range [lo, hi] ground truth g is ignored iff area_g < lo or area_g > hi (both ends inclusive); n_valid = the
 *            ground truths not ignored.  Ground truths are visited non-ignored first, each group in index order.
 *   IoU      inter / (area_d + area_g - inter) as a correctly rounded double (0 where the union is 0), so every comparison below
 *            decides as IEEE double arithmetic on the host does, also for an IoU exactly on a threshold.
 *   match    per threshold t, walking the kept detections in order, bar = min(t, 1 - 1e-10): among the not yet matched non-ignored
 *            ground truths with IoU >= bar the one with the greatest IoU, the LAST in visiting order on a tie; only if there is
 *            none, the same among the not yet matched ignored ones.  The match consumes the ground truth for that threshold.
 *            dt_ignore = 1 iff the detection matched an ignored ground truth, or is unmatched and its own area is outside [lo, hi].
 *   outputs  (device, all overwritten) order_out int32 [max_det] = detection index per rank; match_out int32
 *            [n_ranges][n_thresholds][max_det] = matched ground-truth INDEX or -1; dt_ignore_out uint8 of the same shape;
 *            n_valid_out int32 [n_ranges]; n_kept_out int32 [1].  Ranks >= n_kept hold -1 / -1 / 0.
 * A match is a match by index: ground truth 0 can be matched like any other (pycocotools stores the annotation id and tests it for
 * truth, which loses the matches to id 0 -- and gt_ins_<tag>.json restarts its ids at 0 per image).
 * A null handle / output / needed input, nd or ng < 0, n_thresholds or n_ranges outside 1..16, max_det outside 1..4096, a NaN
 * threshold or bound, or a NaN among host scores: SAMRS_ERR_BAD_ARG, nothing launched.  Device scores cannot be read without a
 * synchronisation: a NaN among them makes the kernel write n_kept = -1 and match nothing.  nd == 0 or ng == 0 is a valid image.
 * One block per area range, one wave per threshold; no host synchronisation.  Scratch: n_ranges * n_thresholds * ng bytes (+ 4 nd
 * for host scores) in ONE buffer per handle that grows on demand: calls on a handle must be stream-ordered with each other (same
 * stream, or an event between them); two handles never share it.
 *
 * Boundary IoU and Boundary AP (Cheng et al., CVPR 2021): mask IoU is dominated by the interior of a large object, so a mask whose
 * outline is a few pixels off still matches at every threshold; these count the band along the outline instead.  The rules below are
 * the definition (the tests pin them to an independent host statement and to scipy.ndimage, not to cv2):
 *   dilation      d = max(1, int(round(ratio * hypot(H, W)))), computed by the caller (samrs_amd.coco_ap.boundary_dilation); the
 *                 usual ratio is 0.02: a 1024 x 1024 tile gives 29, 800 x 1200 gives 29, 45 x 70 gives 2.
 *   band of M     band(M)[y][x] = M[y][x] AND NOT E[y][x], where E[y][x] = 1 iff every pixel of the (2 d + 1) x (2 d + 1) square
 *                 centred on (y, x) lies inside the image and is set in M; everything outside the image counts as background.
 *                 That is d iterations of a 3 x 3 all-ones erosion with a zero border; equivalently the band holds the set pixels
 *                 within Chebyshev distance d of a background pixel or of the image edge.  Where w < 2 d + 1 or h < 2 d + 1 the band
 *                 is the whole mask.
 *   Boundary IoU  of prediction P and ground truth G: |band(P) AND band(G)| / |band(P) OR band(G)|, 0 for an empty union.
 *   Boundary AP   samrs_coco_match's matching and COCO's accumulation with the pair score min(mask IoU, boundary IoU), each IoU a
 *                 correctly rounded double.  Area ranges, the ground truths' ignore flags and the unmatched detection's ignore flag
 *                 still use the MASK areas; order, ties, bar = min(t, 1 - 1e-10) and the match by index are samrs_coco_match's.
 * samrs_mask_boundary_bits: planes uint64 [n][words] in the layout above (from samrs_mask_pack_bits or samrs_label_pack_bits alike)
 *   -> band_out uint64 [n][words], tail bits zero; band_out must not overlap planes.  The square erosion runs as a horizontal and a
 *   vertical pass on the packed bits, 64 pixels per lane operation; rows need not be word-aligned and a word may hold several rows.
 *   One writer per output word, no atomics: deterministic.  A null handle or pointer, n < 0, h or w < 1, h * w >= 2^30, d outside
 *   1..128 or an output that overlaps the input: SAMRS_ERR_BAD_ARG with nothing launched or written.  n == 0 is a no-op.  The
 *   row-eroded planes live in ONE scratch per handle that grows on demand (8 bytes per word, at most 64 MiB: more masks are
 *   banded in several passes): calls on a handle must be stream-ordered with each other.
 * samrs_coco_match_min: samrs_coco_match with a second triple inter_b int64 [nd][ng], area_db int64 [nd], area_gb int64 [ng] -- the
 *   samrs_mask_pair_counts of the two stacks' bands -- and the pair IoU replaced by min(IoU(inter, area_d, area_g), IoU(inter_b,
 *   area_db, area_gb)).  The second triple is needed wherever the first is (else SAMRS_ERR_BAD_ARG); everything else, the scratch
 *   and its stream-ordering rule included, is samrs_coco_match's, which itself is unchanged. */
int samrs_mask_boundary_bits(samrs_engine_t* e, const uint64_t* planes, int n, int h, int w, int d, uint64_t* band_out, void* stream);
int samrs_coco_match_min(samrs_engine_t* e, const int64_t* inter, const int64_t* area_d, const int64_t* area_g, const int64_t* inter_b,
                         const int64_t* area_db, const int64_t* area_gb, const float* scores, int scores_on_host, int nd, int ng,
                         const double* thresholds, int n_thresholds, const double* area_ranges, int n_ranges, int max_det,
                         int32_t* order_out, int32_t* match_out, uint8_t* dt_ignore_out, int32_t* n_valid_out, int32_t* n_kept_out,
                         void* stream);
int samrs_mask_pack_bits(samrs_engine_t* e, const uint8_t* masks, int n, int h, int w, uint64_t* planes_out, void* stream);
int samrs_label_pack_bits(samrs_engine_t* e, const uint8_t* label_rgb, const uint8_t* colors, int n, int h, int w, uint64_t* planes_out,
                          void* stream);
int samrs_mask_pair_counts(samrs_engine_t* e, const uint64_t* a, int na, const uint64_t* b, int nb, int64_t words, int64_t* inter_out,
                           int64_t* area_a_out, int64_t* area_b_out, void* stream);
int samrs_coco_match(samrs_engine_t* e, const int64_t* inter, const int64_t* area_d, const int64_t* area_g, const float* scores,
                     int scores_on_host, int nd, int ng, const double* thresholds, int n_thresholds, const double* area_ranges,
                     int n_ranges, int max_det, int32_t* order_out, int32_t* match_out, uint8_t* dt_ignore_out, int32_t* n_valid_out,
                     int32_t* n_kept_out, void* stream);

/* -- the generation CLI's class-map files (main_sam_hbox_semantic.py:212-215: gray/<stem>.png and color/<stem>.png), encoded on
 * the device.  maps: uint8 [n][h][w] (255 = unlabeled), lut: uint8 [256][3] (class id -> RGB), both on the device.  The two PNG
 * files of each map are byte-identical with what the host's samrs_io_png_write_label_pair (include/samrs_io.h) writes for
 * (maps[i], lut).  Same buffer protocol as samrs_rle_encode: the files are packed into `out` (device bytes, 16-byte aligned,
 * capacity out_capacity) at 16-byte aligned offsets behind *cursor (device int64, in / out), and table [n][2][2] (device int64)
 * receives (offset, length) of the gray and the colour file of each map; length < 0 means the file did not fit (-length - 1 bytes
 * were needed) and was not written.  h, w <= 65536 and (3 w + 1) h < 2^31.  No host synchronisation; the token scratch lives in
 * ONE buffer per handle: all samrs_png_encode_labels calls on a handle must be stream-ordered with each other. */
int samrs_png_encode_labels(samrs_engine_t* e, const uint8_t* maps, int n, int h, int w, const uint8_t* lut, uint8_t* out,
                            int64_t out_capacity, int64_t* cursor, int64_t* table, void* stream);

/* -- visualize.py's overlays (Image.blend(image, seg_color, 0.4) saved under vis/), on the device.
 * samrs_blend_labels: out = blend(images, lut[maps], alpha) for n images uint8 [n][h][w][3] and their class maps uint8 [n][h][w]
 * through lut uint8 [256][3] (class id -> RGB), all on the device; out uint8 [n][h][w][3] must not alias images.  Bit-exact with
 * Pillow's Image.blend for 0 <= alpha <= 1: per byte (uint8)((int)a + alpha * ((int)b - (int)a)) in float arithmetic, the product
 * and the sum each rounded to float, the result truncated.  Any h, w >= 1.  alpha outside [0, 1] (or NaN), n, h or w < 1, a null
 * pointer: SAMRS_ERR_BAD_ARG, nothing launched.  No host synchronisation, no scratch.
 *
 * samrs_png_encode_rgb: n images uint8 [n][h][w][3] on the device -> n complete PNG files (8-bit colour type 2, not interlaced, one
 * IDAT; zlib header 78 9c; the filtered bytes as literals of dynamic-Huffman blocks of SAMRS_PNG_RGB_BLOCK_BYTES filtered bytes, no
 * LZ77 matches).  filter 0 .. 4 forces that PNG row filter on every row; -1 chooses per row the filter with the least sum of the
 * filtered bytes' magnitudes as int8 (v < 128 ? v : 256 - v; the filter byte itself not counted), the lowest number on a tie.  The
 * bytes of a file are a function of its pixels and `filter` alone.  Same buffer protocol as samrs_png_encode_labels: the files are
 * packed into `out` (device bytes, 16-byte aligned, capacity out_capacity) at 16-byte aligned offsets behind *cursor (device int64,
 * in / out), and table [n][2] (device int64) receives (offset, length) per image; length < 0 means the file did not fit (-length - 1
 * bytes were needed), nothing of it was written and the cursor did not move for it.  h, w <= 65536 and (3 w + 1) h < 2^31.
 * Worst-case file size, to size `out`: with N = (3 w + 1) h filtered bytes in B = ceil(N / SAMRS_PNG_RGB_BLOCK_BYTES) blocks,
 *     63 + ceil((9 N + B (4498 + 9)) / 8) bytes,
 * rounded up to a multiple of 16 per file in the buffer: an optimal prefix code over a block's <= 257 symbols costs no more than the
 * 9-bit fixed code, and a block adds a header of <= 4498 bits; 63 bytes are framing.  The bound holds whenever no code would be
 * longer than deflate's 15 bits (every image whose rarest byte value is not rarer than about 1 in 2^15 of a block); where the
 * length limit steps in, the code is no longer optimal and only 15 bits per byte are guaranteed -- such data is far below the bound
 * in practice, and a file that does not fit is reported, never truncated.
 * No host synchronisation; the filtered bytes and code tables live in ONE scratch buffer per handle (8 images per pass, about
 * (3 w + 1) h bytes each), so all samrs_png_encode_rgb calls on a handle must be stream-ordered with each other. */
#define SAMRS_PNG_RGB_BLOCK_BYTES 1048576
int samrs_blend_labels(samrs_engine_t* e, const uint8_t* images, const uint8_t* maps, const uint8_t* lut, float alpha, uint8_t* out, int n,
                       int h, int w, void* stream);
int samrs_png_encode_rgb(samrs_engine_t* e, const uint8_t* rgb, int n, int h, int w, int filter, uint8_t* out, int64_t out_capacity,
                         int64_t* cursor, int64_t* table, void* stream);

/* -- "next row" N3: one separable pass of Pillow's 8-bit resample (ResizeLongestSide.apply_image,
 * utils/transforms.py:26-31 -> PIL Image.resize BILINEAR).  `bounds` int32 [out_len,2] = (first input
 * index, tap count), `coef` int32 [out_len,ksize] 22-bit fixed point, both computed on the host exactly
 * as Pillow does (samrs_amd/transforms.py).  horizontal: in [other,in_len,3] -> out [other,out_len,3];
 * vertical: in [in_len,other,3] -> out [out_len,other,3].  Bit-exact with PIL. */
int samrs_resample_pass_u8(const uint8_t* in, uint8_t* out, const int32_t* bounds, const int32_t* coef,
                           int ksize, int in_len, int out_len, int other, int horizontal, void* stream);

/* -- per-engine options (each handle has its own; the environment variable named in brackets only sets the value a NEW handle
 * starts with).  Returns SAMRS_ERR_BAD_ARG for an unknown name.
 *   "split"          [SAMRS_SPLIT; default 79 where the one-launch split GEMM covers the block shapes (ViT-H), else 15] bit mask of
 *                    the rounding points that run as a two-term operand split (hi + lo, three MFMAs, ~2^-22 operand error
 *                    instead of 2^-11): 1 = patch embed, 2 = neck, 4 = decoder image->token out-projection, 8 = decoder upscaler
 *                    (both transposed convs).  15 = every block GEMM at the 1x f16 rate: enough for IoU >= 0.9995 on the single
 *                    mask of token 0 (what the hbox-semantic path asks for); 0 = the round-2 engine's arithmetic.
 *                    Block-GEMM bits: 64 = the v third of the qkv product + proj (q and k pass through the softmax), 16 = all of
 *                    qkv + proj, 32 = the MLP GEMMs (63 / 127 = every MFMA operand of the path), 128 = lin2 alone of the MLP GEMMs
 *                    ("lo_format" 4 only; 207 = 79 | 128 is the error budget's cheapest mode with more margin on the multimask
 *                    outputs: oracle/error_budget.py plans10).  With "lo_format" 4 a split GEMM costs 1.25 - 1.8x a plain one (f16 lo
 *                    terms: 3x).  79 = 15 | 64 holds IoU >= 0.999 on the three multimask tokens too (0.9992 on 192 masks) at 0.92x
 *                    the throughput of 15 and is what a ViT-H handle starts with.  The block-GEMM bits need lo copies of the
 *                    block weights: set them BEFORE samrs_finalize_weights; they can be cleared and set again afterwards.
 *                    What each bit buys in mask pixels: oracle/error_budget.py, DESIGN.md 2.
 *   "split_depth"    [SAMRS_SPLIT_DEPTH, default 0 = automatic] the block-GEMM bits apply to the first N encoder blocks only: an
 *                    operand error made in an early block is carried through every later one, one made in the last blocks is
 *                    not.  Automatic: every block for 16 / 32, the leading three quarters (24 of 32) for 64.
 *   "decoder_fusion" [SAMRS_DECODER_FUSION, default 1] 0 = run the decoder with its un-fused kernels (separate GEMM / LayerNorm /
 *                    product launches; never split): the fused-vs-unfused parity test and timing experiments.
 *   "ln_fold"        [SAMRS_LN_FOLD, default 0] (EXPERIMENTS builds only; embed_dim 1280; only while no block-GEMM bit of "split" is set) 1 = fold the encoder blocks' LayerNorms into the qkv / lin1
 *                    GEMMs.  Measured slower on MI355X.  Must be on before samrs_finalize_weights for the folded weights to
 *                    exist; can be flipped afterwards.
 *   "gemm_variant"   [default -1 = automatic] GEMM tile variant for this handle's launches (tools/gemm_bench.py lists them).
 *   "decode_prompts" [default max_prompts] prompts ONE decoder chain of samrs_predict_multi may hold: every per-prompt decoder workspace
 *                    is sized by it.  Accepted: max_prompts <= value <= min(max_images x max_prompts, 512), anything else is
 *                    SAMRS_ERR_BAD_ARG.  512 is what the index types carry: up to there every element index and byte offset of a chain
 *                    stays below 2^31 (n x 4096 x 384 key-projection elements pass it at n = 1366, n x 2^22 bytes of fp32 keys at 512).
 *                    Set before samrs_finalize_weights it sizes the first allocation; set later it reallocates the workspaces at
 *                    once, on the calling thread: the device is synchronised before a replaced buffer is released, an allocation
 *                    that fails leaves the engine as it was (SAMRS_ERR_HIP), and no chain may be running on another thread.  The
 *                    workspaces never shrink; a lower value only shortens the chains.  Memory per prompt at 16 tokens x 4096 x
 *                    256: 12 bytes per key element (fp32 keys 4, operand keys 2, their split remainder 2, projections 3, attention
 *                    output 1) = 12.6 MB, 0.8 MB of low-res logits, 0.2 MB on the token side: 13.5 MB, 3.5 GB at 256 prompts.  A
 *                    mask prompt adds 4.2 MB per prompt, the upscaler forms other than the one-kernel one 10.5 MB (first use).
 *                    samrs_predict is not affected: it decodes max_prompts per pass, as it always did.  Results do not depend on
 *                    the chain length, bit for bit.
 *   "decode_kbytes"  read-only: KiB of per-prompt decoder workspace allocated now (the byte count does not fit an int).
 *   "upscaler_fused" [SAMRS_UPSCALER_FUSED, default 1] 1 = the mask upscaler as ONE kernel (samrs_k_upscaler_fused); 0 = ConvT #1 as a GEMM with a
 *                    LayerNorm2d + GELU epilogue, then the ConvT #2 + GELU + product kernel (A/B runs, tests).
 *   "split_passes"   [SAMRS_SPLIT_PASSES, default 0] reference-grade bits of "split" only: 1 = the three terms of a split block GEMM as
 *                    three accumulating launches through an fp32 scratch (the generic route, every shape); 0 = as ONE launch over a
 *                    three-segment K axis where the shape fits the 256 x 320 tile (ViT-H; samrs_k_gemm_split3), else the generic route.
 *   "lo_format"      [SAMRS_LO_FORMAT; default 4 where the MX kernel covers the block shapes (ViT-H), else 0] operand format of the two
 *                    correction terms of the block-GEMM split (bits 64 / 16 and 32): 0 = f16 (a split GEMM is three f16
 *                    passes), 4 = MXFP4 (e2m1 + E8M0 scale per 32 k on gfx950's block-scaled MFMA: the corrections run at 4x the f16
 *                    rate on a quarter of the stages, a split GEMM costs 1.5 passes; oracle/error_budget.py plans10 for what the
 *                    format costs in mask pixels: nothing measurable).  The fp4 weight copies are made at samrs_finalize_weights
 *                    when a block-GEMM bit is set by then; afterwards the option can be flipped between 0 and 4 (A/B runs).
 *   "allow_reduced"  [SAMRS_ALLOW_REDUCED; default 0, 1 when SAMRS_SPLIT is set] 1 = samrs_predict(multimask = 1) accepts embeddings
 *                    encoded below the multimask grade (see samrs_get_slot_info) instead of returning SAMRS_ERR_PRECISION.
 *   "gelu_fast"      [SAMRS_GELU_FAST, default -1 = automatic] erf of the GELU in lin1's epilogue (image_encoder.py:177-180, common.py:18-26;
 *                    168 M elements per launch at ViT-H): 0 = Abramowitz-Stegun 7.1.26 (|error| <= 1.5e-7: fp32-epsilon class, two
 *                    transcendentals per element), 1 = 7.1.28 (|error| <= 3e-7, one v_rcp_f32 and no exp2: -3.3 % on the dominant
 *                    kernel; both are three orders of magnitude under the f16 rounding the value receives next).  Automatic: 1 in the
 *                    1x-rate modes ("split" without a block-GEMM bit: what the single-mask pipelines run), 0 in every reference-grade
 *                    mode, whose arithmetic stays bit for bit what its committed parity statistics were measured on.  Applies where
 *                    lin1 runs on the persistent 256 x 320 kernel (ViT-H shapes); elsewhere the option has no effect.
 *   "ln_tail"        [SAMRS_LN_TAIL, default 0] 1 = the LayerNorm that follows proj (norm2, image_encoder.py:177) and lin2 (norm1 of the
 *                    next block, :168) runs as a TAIL of those GEMM launches instead of a launch of its own: the block that stores the
 *                    last of the four 256 x 320 tiles of a 256-row panel normalises the panel's rows (release / counter / acquire between
 *                    the four blocks, nobody waits: gemm.hip LnTail).  Bit-identical with the stand-alone LayerNorm, and measured SLOWER
 *                    (61.8 against 57.2 ms per 8-tile step): one CU draws ~20 GB/s from HBM, so a panel takes it 62 us where a LayerNorm
 *                    launch on all 256 CUs takes 53 for the whole tensor (profiles/r05_ln_tail.txt).  Kept as an option for the record
 *                    and for its test; 1x-rate modes only, batches of 4+ tiles at ViT-H.
 *   "operand_pad"    [SAMRS_OPERAND_PAD, default 1; read at samrs_finalize_weights for the copies, switchable afterwards] ViT-H: the K = 1280
 *                    operands of the plain qkv / lin1 launches -- the LayerNorm output and the weights -- are stored with a row stride of 1408
 *                    elements (2816 B = eleven 256-byte units) instead of 1280 (ten units: the 256 rows a tile fetches per k-slice then fall
 *                    on half of the memory channels); the persistent ET kernels read A and B with that stride.  Costs 0.8 GB for the padded
 *                    weight copies.  Only where the bytes live changes: bit-identical output in every mode.
 *   "range_check"    [SAMRS_RANGE_CHECK, default 0] the f16 operand type has 11 mantissa bits (what the IoU >= 0.999 bar needs) but
 *                    tops out at 65504, and every conversion on the path SATURATES there instead of overflowing to inf -- silently.
 *                    1 = after each producer of an MFMA-operand tensor in the encoder (both LayerNorm outputs, q | k | v, the
 *                    attention output, GELU(lin1), the residual stream in front of the neck, the neck's LayerNorm2d output, the
 *                    decoder's layer-0 keys) a scan adds the number of elements at the saturation value (or inf / nan) to a
 *                    per-engine counter, read -- and, by writing any value, reset -- through the option "saturated"; ~7 extra
 *                    passes over those tensors per block (+ 25 % encoder time): a validation mode for a NEW CHECKPOINT, not the
 *                    production setting.  2 = the same, and samrs_set_images* returns SAMRS_ERR_RANGE when its pass saturated
 *                    anything (one stream synchronisation per pass).  The remedy is the bf16 operand type (fp32 exponent range;
 *                    misses the IoU bar by its 8 mantissa bits: DESIGN.md 2) -- there is no silent fallback.
 *   "saturated"      read: the counter of "range_check" (clamped to INT_MAX; synchronizes the device); write: reset.
 *   "outlier_cols"   [SAMRS_OUTLIER_COLS, default 7 = bit 0 (qkv / lin1) | bit 1 (lin2) | bit 2 (proj); non-zero at samrs_finalize_weights
 *                    for the picking, switchable afterwards] checkpoint
 *                    weights have outlier channels (a few LayerNorm gammas 10 - 100x the rest, hidden units / v channels that run
 *                    thousands of times hotter), and an f16 operand's rounding error is relative to ITS magnitude: those few K-columns
 *                    carry most of the operand error of a block GEMM.  At load time every block GEMM's columns are scored from the
 *                    fp32 weights alone (operand magnitude proxy x weight column norm); those above "outlier_ratio_pct" of the
 *                    median score (at most 32 per GEMM) are its outlier columns.  For the plain qkv / lin1 launches their hi + lo
 *                    split rides as 64 more K columns of the SAME launch (the LayerNorm writes the operand side, the weights carry
 *                    the matching columns): + 1 / 20 of those two GEMMs in the blocks that have such columns, nothing elsewhere.
 *                    lin2 / proj read operands that other kernels write, so their 64 columns travel as a dense side operand
 *                    ([M][64]: the attention kernel's lo output gathered for proj; for lin2 the outlier hidden units recomputed
 *                    in fp32 by a 128-column side GEMM, exact GELU, split) and enter as one more K stage of the same launch.
 *                    Weights without outliers (seeded-normal test models) pick nothing: bit-identical output, zero cost.
 *   "outlier_ratio_pct" [SAMRS_OUTLIER_RATIO_PCT, default 400; before samrs_finalize_weights only]
 *   "outlier_blocks" / "outlier_columns" / "outlier_dominant_blocks"  read-only: encoder blocks with at least one outlier column in
 *                    qkv / lin1; the number of columns picked over all four block GEMMs; blocks in which the picked columns carry more
 *                    than half of the qkv or proj operand-error mass -- in the v-third modes (79 / 207) those blocks run the plain
 *                    launches with the exact lo terms of their outlier columns instead of the MXFP4 lo terms of all columns.
 *   "range_profile"  [SAMRS_RANGE_PROFILE, default 0] the checkpoint audit (samrs_audit_* below).  1 = on every encoder pass each audit
 *                    SITE -- the operand tensors "range_check" scans, q | k | v apart -- adds its range profile (counts of zeros,
 *                    subnormals, saturated values, inf / nan, the largest magnitude, a histogram of floor(log2 |x|)) to a per-site row on
 *                    the device; 2 = the same plus, for the A operand of every block GEMM, per-column sum of squares and largest magnitude
 *                    (what "outlier_cols" guesses from the weights, measured).  One more pass over those tensors (two with 2): a
 *                    validation mode.  Independent of "range_check"; every "split" mode and both operand types.  0 launches nothing.
 *   "audit_passes"   [SAMRS_AUDIT_PASSES, default 0] write N > 0: reset the audit state, set "range_profile" = 2 and profile the next N
 *                    encoder passes (samrs_set_images* calls); the engine then sets "range_profile" back to 0 by itself, so the steady
 *                    state launches nothing extra.  Read: passes left.  Write 0: stop a running audit. */
int samrs_set_option(samrs_engine_t* e, const char* name, int value);
int samrs_get_option(const samrs_engine_t* e, const char* name, int* value);

/* -- checkpoint audit: where in the encoder do the operand tensors sit in the operand type's range, and which K-columns of the block GEMMs
 * are really hot (options "range_profile" / "audit_passes"; python -m samrs_amd.audit prints the report).
 * Sites, in data-flow order, 7 depth + 3 of them (fixed at samrs_finalize_weights; 0 sites before): per encoder block i
 * "blocks.i.qkv_in" (norm1 output), "blocks.i.q", "blocks.i.k", "blocks.i.v", "blocks.i.proj_in" (attention output), "blocks.i.lin1_in"
 * (norm2 output), "blocks.i.lin2_in" (GELU(lin1)); then "neck.conv1_in" (the residual stream rounded to the operand type), "neck.conv2_in",
 * "decoder.keys0".  samrs_audit_site_name copies the name (truncated to name_len - 1 characters) and, if `columns` is not NULL, the K of
 * the site's column statistics (qkv_in, proj_in, lin1_in: embed_dim; lin2_in: 4 embed_dim; every other site 0 = none).
 * A profile row is 48 int64, accumulated over the profiled passes:
 *   [0] elements scanned   [1] zeros   [2] subnormals of the operand type (f16: 0 < |x| < 2^-14)   [3] elements AT the largest finite
 *   magnitude (f16 0x7bff = 65504, what the saturating conversions write)   [4] inf or nan   [5] the largest finite magnitude seen as its
 *   15-bit pattern `bits & 0x7fff` (a running maximum)   [6], [7] zero   [8 + b], b = 0 .. 39: finite non-zero elements with
 *   floor(log2 |x|) == b - 24, clamped into [-24, 15] (f16 covers exactly this range; bf16 clamps at both ends).
 *   [1] + [4] + sum of the bins == [0]; the elements of [2] and [3] are also in their bins.
 * samrs_audit_read_profile copies all rows to HOST memory and samrs_audit_read_columns one site's column statistics (sumsq [K] = sum of
 * x^2 over the n_rows rows seen, max_abs [K]; a bf16 magnitude above 1.8e19 makes its column's sum inf); both synchronise the device
 * (diagnostics, like option "saturated").  All sums are integer atomics or ordered fp64 sums of fp32 partials: bitwise reproducible.
 * reset != 0 clears the whole audit state (rows and column statistics) after the copy.  samrs_audit_read_columns returns
 * SAMRS_ERR_BAD_ARG for a site without column statistics, or when no pass has been profiled with "range_profile" = 2 since the last reset. */
int samrs_audit_site_count(const samrs_engine_t* e, int* n_sites);
int samrs_audit_site_name(const samrs_engine_t* e, int site, char* name, int name_len, int* columns);
int samrs_audit_read_profile(samrs_engine_t* e, int64_t* rows, int reset);
int samrs_audit_read_columns(samrs_engine_t* e, int site, double* sumsq, float* max_abs, int64_t* n_rows);

/* Rotated-box MASK prompts, replacing the cv2 pre-step of `Generate Dataset/main_sam_rbox_mask_instance.py:125-141`
 * (fillPoly -> +-1000 -> resize to the ResizeLongestSide shape -> pad with -1000 -> resize to 256x256).
 * pts: device int32 [n][n_vertices][2] (x, y) in ORIGINAL image pixels (the reference's `.astype(np.int32)`),
 * 3 <= n_vertices <= 8; (h, w) original size; (th, tw) = ResizeLongestSide.get_preprocess_shape(h, w, img_size);
 * out: device fp32 [n][out_size][out_size] = the `mask_input` of samrs_predict (out_size = 256). */
int samrs_rbox_mask_prompt(const int32_t* pts, int n, int n_vertices, int h, int w, int th, int tw,
                           int img_size, int out_size, float* out, void* stream);
/* The same with the polygon fill rule named.  cv2.fillPoly's scanline spans changed in OpenCV 4.5.2 (modules/imgproc/src/drawing.cpp
 * FillEdgeCollection): up to 4.5.1 a span covers ceil(x_left) .. floor(x_right) of the 16.16 fixed-point edge crossings, since 4.5.2
 * both ends are rounded half up; the 8-connected boundary lines drawn on top are the same.  The reference pins no OpenCV version
 * (`Generate Dataset/main_sam_rbox_mask_instance.py:126-129`), and on FAIR1M-shaped boxes ~18 % of the polygons differ by 1 - 8
 * boundary pixels between the two, so the caller says which cv2 it replaces (samrs_amd.transforms picks by cv2.__version__ when
 * cv2 is importable).  samrs_rbox_mask_prompt == fill_rule SAMRS_FILL_CV2_LE_451. */
enum samrs_fill_rule { SAMRS_FILL_CV2_LE_451 = 0, SAMRS_FILL_CV2_GE_452 = 1 };
int samrs_rbox_mask_prompt_rule(const int32_t* pts, int n, int n_vertices, int h, int w, int th, int tw,
                                int img_size, int out_size, int fill_rule, float* out, void* stream);

/* The kernel-level entry points (samrs_k_*) and the test / measurement hooks (samrs_debug_*) that the parity tests, bench.py's
 * in-situ kernel timer and the tools/ scripts use are declared in samrs_hip_internal.h: exported by the same library, NOT part of
 * the drop-in boundary, and without any compatibility promise. */

#ifdef __cplusplus
}
#endif
#endif /* SAMRS_HIP_H */
