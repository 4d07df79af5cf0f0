#!/usr/bin/env python3
"""What Boundary AP costs, three arms alternating in one process, one JSON line per run.

  ap        InstancePipeline(gt=True, ap=True): images/s over `--steps` steps of 8 x 1024^2 tiles, 32 rotated boxes each (rle=True, the
            box prompt, single mask) -- tools/coco_ap_bench.py's loop.
  boundary  the same with boundary=True: both plane stacks banded (d = 29), a second pair count and the min-matching per tile.
  band      the band kernels alone, device events: Engine.mask_boundary_bits on the planes of 32 seeded ellipses of one 1024^2 tile,
            d = 29, next to Engine.pack_mask_bits on the same masks, `--calls` calls each.

Every arm runs once unmeasured, then `--reps` times in turn.  The last line is the per-tile cost of boundary=True over the ap arm of
the same run.
With --out the lines are also appended to that file (profiles/boundary_ap_bench.txt keeps a run).
usage: boundary_ap_bench.py [--calls 20] [--steps 12] [--reps 2] [--model vit_h] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import samrs_amd  # noqa: E402
from samrs_amd import coco_ap, driver, synth  # noqa: E402
from coco_ap_bench import BATCH, BOXES, SIDE, ellipses, items, timed  # noqa: E402


def run_pipeline(sam, work, boundary):
    pipe = driver.InstancePipeline(sam, 1, prompt="box", multimask=False, gt=True, ap=True, boundary=boundary, batch=BATCH, box_batch=BOXES,
                                   max_boxes=BOXES, rle=True)
    band = [0]

    def sink(res, rel):
        band[0] += sum(int(r.band_area_d.sum()) for r in res if r.band_area_d is not None)
        rel()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = pipe.run(driver.batched(work, BATCH), sink)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"arm": "boundary" if boundary else "ap", "images": n, "images_per_s": round(n / dt, 1), "seconds": round(dt, 4),
            "ms_per_tile": round(dt / max(n, 1) * 1e3, 4), "band_pixels_per_image": round(band[0] / max(n, 1), 1)}


def run_band(eng, masks, planes, out, d, calls):
    pack = [timed(lambda: eng.pack_mask_bits(masks, planes)) for _ in range(calls)]
    band = [timed(lambda: eng.mask_boundary_bits(planes, SIDE, SIDE, d, out)) for _ in range(calls)]
    words = planes.shape[1]
    return {"arm": "band", "masks": int(masks.shape[0]), "tile": [SIDE, SIDE], "d": d, "band_ms_median": round(float(np.median(band)), 4),
            "band_ms_min": round(min(band), 4), "pack_mask_bits_ms_median": round(float(np.median(pack)), 4),
            "pack_mask_bits_ms_min": round(min(pack), 4), "plane_bytes": int(masks.shape[0]) * words * 8,
            "band_pixels": int(eng.mask_pair_counts(out, out)[1].sum())}


def emit(rec: dict, path) -> None:
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also append every JSON line to this file")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--model", default="vit_h")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("boundary_ap_bench.py measures on the GPU: no HIP device found")
    sd = synth.make_state_dict(synth.CONFIGS[a.model], 0, logit_scale=synth.MARGIN_LOGIT_SCALE)
    sam = samrs_amd.sam_model_registry[a.model](state_dict=sd, precision="f16", max_images=2 * BATCH, max_prompts=64, max_points=1).to("cuda")
    eng = sam.engine
    work = items(a.steps * BATCH)
    masks = ellipses(BOXES, 11)
    d = coco_ap.boundary_dilation(SIDE, SIDE)
    planes = eng.pack_mask_bits(masks)
    out = torch.empty_like(planes)
    for arm in (False, True):                                      # unmeasured first run per arm
        run_pipeline(sam, work[:3 * BATCH], arm)
    run_band(eng, masks, planes, out, d, 2)
    per_tile = {"ap": [], "boundary": []}
    for rep in range(a.reps):
        for arm in (False, True):
            r = run_pipeline(sam, work, arm)
            r["rep"], r["model"] = rep, a.model
            per_tile[r["arm"]].append(r["ms_per_tile"])
            emit(r, a.out)
        r = run_band(eng, masks, planes, out, d, a.calls)
        r["rep"] = rep
        emit(r, a.out)
    base, on = float(np.median(per_tile["ap"])), float(np.median(per_tile["boundary"]))
    emit({"boundary_over_ap_ms_per_tile": round(on - base, 4), "ap_ms_per_tile": round(base, 4), "boundary_ms_per_tile": round(on, 4),
          "relative": round((on - base) / base, 4), "model": a.model}, a.out)
    eng.close()


if __name__ == "__main__":
    main()
