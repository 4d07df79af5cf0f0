"""GPU: sha256 of everything the three product pipelines hand to their sinks, through the public surface only (constructors, run,
TileResult fields, class_pixels / class_instances), so that the same file runs against two checkouts: two trees that print the same
lines compute the same outputs.  One line per (configuration, key, non-None TileResult field) and one per statistics vector.
vit_tiny with seeded weights of a checkpoint-like logit spread, one 1024^2 and one 600 x 800 tile of 4 boxes each (batch 2, chunks
of 3 boxes): TilePipeline plain, with each output alone, and with all of them and a stability threshold that drops half of the
instances, each with batch_decode off / on and keep_masks off / on; InstancePipeline(gt, rle, mask_boxes, min_region_area) for the
three prompt kinds, multimask on / off, batch_decode off / on; ScenePipeline on a 256 x 448 scene in two windows with every output.
The packed byte buffers (pinned, reused, with alignment gaps) are hashed as the strings and files their tables cut out of them.
usage: pipeline_hash.py [TREE]     TREE: the checkout to import samrs_amd from (default: this one); SAMRS_LIB_PATH names the library"""
import dataclasses
import hashlib
import os
import sys

import numpy as np

TREE = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)
import samrs_amd  # noqa: E402
from samrs_amd import driver, quality, synth, tile_io  # noqa: E402
from samrs_amd.scene import ScenePipeline  # noqa: E402

assert os.path.abspath(samrs_amd.__file__).startswith(TREE + os.sep), samrs_amd.__file__
SIZES = [(1024, 1024), (600, 800)]
N_CLASSES = 18


def sha(*parts) -> str:
    h = hashlib.sha256()
    for p in parts:
        h.update(p if isinstance(p, bytes) else repr(p).encode())
    return h.hexdigest()[:16]


def field_digests(r) -> dict:
    n, out = len(r.labels), {}
    for f in dataclasses.fields(r):
        v = getattr(r, f.name)
        if v is None or f.name == "key":
            continue
        if f.name == "rle_data":
            v = [r.rle(j) for j in range(n)]
        elif f.name == "gt_rle_data":
            v = [r.gt_rle(j) for j in range(n)]
        elif f.name == "png_data":
            v = [bytes(r.png("gray")), bytes(r.png("color"))]
        out[f.name] = sha(str(v.dtype), v.shape, np.ascontiguousarray(v).tobytes()) if isinstance(v, np.ndarray) else sha(v)
    return out


def run(name, pipe, batches, keep=None):
    def sink(results, release):
        for r in results:
            for f, d in field_digests(r).items():
                print(f"{name} | {r.key} | {f} {d}", flush=True)
            if keep is not None:
                keep.append(r.score_counts.copy())
        release()
    pipe.run(batches, sink)
    for f in ("class_pixels", "class_instances"):
        print(f"{name} | {f} {sha(getattr(pipe, f).cpu().numpy().tobytes())}", flush=True)


weights = synth.make_state_dict(synth.CONFIGS["vit_tiny"], 0, logit_scale=synth.MARGIN_LOGIT_SCALE)
sam = samrs_amd.sam_model_registry["vit_tiny"](state_dict=weights, max_images=4, max_prompts=20, precision="f16").to("cuda")
lut = tile_io.class_lut(np.random.default_rng(2).integers(0, 256, (N_CLASSES, 3), dtype=np.uint8))
KW = dict(batch=2, box_batch=3, max_boxes=8)

# ---- TilePipeline -------------------------------------------------------------------------------------------------------------
tiles = []
for i, (h, w) in enumerate(SIZES):
    boxes, labels = synth.make_boxes(60 + i, 4, h, w)
    tiles.append(driver.WorkItem(f"B{i:04d}", synth.make_image(60 + i, h, w), boxes, labels))
counts = []
run("tile probe quality", driver.TilePipeline(sam, N_CLASSES, quality=True, **KW), driver.batched(tiles, 2), counts)
thr = float(np.median(np.concatenate([quality.stability(c) for c in counts])))
print(f"min_stability {thr!r}")
ALONE = {"rle": dict(rle=True, rle_buffer_mb=64), "png_lut": dict(png_lut=lut), "min_region_area": dict(min_region_area=16),
         "mask_boxes": dict(mask_boxes=True), "quality": dict(quality=True),
         "polygons": dict(polygons=True, polygon_buffer_mb=64, polygon_max_edges=1 << 21)}
CONFIGS = {"plain": {}, **ALONE, "all": dict(min_stability=thr, **{k: v for kw in ALONE.values() for k, v in kw.items()})}
for cname, ckw in CONFIGS.items():
    for bd in (False, True):
        for km in (False, True):
            run(f"tile {cname} batch_decode {int(bd)} keep_masks {int(km)}",
                driver.TilePipeline(sam, N_CLASSES, batch_decode=bd, keep_masks=km, **KW, **ckw), driver.batched(tiles, 2))

# ---- InstancePipeline ---------------------------------------------------------------------------------------------------------
objects = []
for i, (h, w) in enumerate(SIZES):
    polys, labels = synth.make_rboxes(60 + i, 4, h, w)
    cols = np.random.default_rng(70 + i).integers(0, 256, size=(4, 3), dtype=np.uint8)
    label = np.full((h, w, 3), 128, dtype=np.uint8)                 # ground truth: each object's enclosing hbox in its colour
    for p, c in zip(polys, cols):
        x0, y0 = np.clip(np.floor(p.min(0)).astype(int), 0, None)
        x1, y1 = np.ceil(p.max(0)).astype(int)
        label[y0:y1, x0:x1] = c
    objects.append((f"R{i:04d}", synth.make_image(60 + i, h, w), polys, labels, (label, cols)))
for prompt in ("box", "rbox_mask", "point"):
    items = [driver.WorkItem(k, img, polys.mean(1).astype(np.float32) if prompt == "point" else polys, labels, gt)
             for k, img, polys, labels, gt in objects]
    for mm in (False, True):
        for bd in (False, True):
            run(f"instance {prompt} multimask {int(mm)} batch_decode {int(bd)}",
                driver.InstancePipeline(sam, 1, prompt=prompt, multimask=mm, gt=True, rle=True, rle_buffer_mb=64, mask_boxes=True,
                                        min_region_area=16, batch_decode=bd, **KW), driver.batched(items, 2))

# ---- ScenePipeline ------------------------------------------------------------------------------------------------------------
H, W = 256, 448
scene_boxes = np.array([[20, 30, 120, 200], [300, 40, 430, 180], [330, 100, 440, 250], [10, 10, 60, 60]], dtype=np.float32)
run("scene every output", ScenePipeline(sam, N_CLASSES, window=256, overlap=64, batch=2, box_batch=3, rle=True, rle_buffer_mb=16, png_lut=lut,
                                        mask_boxes=True, polygons=True, polygon_buffer_mb=16, polygon_max_edges=1 << 21, min_region_area=16),
    [driver.WorkItem("scene", synth.make_image(33, H, W), scene_boxes, np.array([1, 2, 3, 4]))])
sam.engine.close()
