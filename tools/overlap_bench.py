#!/usr/bin/env python3
"""The overlap stage measured two ways, arms alternating in one process, one JSON line per result.

The kernel: samrs_resolve_overlaps (rule LOGIT, removed_out only) on 32 and 64 decoded masks of one 1024^2 tile, beside samrs_paint and
samrs_scene_claim on the same masks -- the two kernels that also read the n h w mask bytes once.  Device events around each call,
`--calls` rounds of paint -> scene_claim -> resolve; the masks are restored from a copy before every call, outside the timed
window.  Two mask sets per n: "decoded" = the masks as the box-prompted decoder of a seeded vit_tiny returns them (seeded weights
paint far outside their boxes: most pixels are contested), and "boxed" = the same masks clipped to their prompt boxes, which is what a
trained SAM's box-prompted masks look like (few contested pixels: the uncontested fast path).  Every line carries the share of
contested pixels, the n h w bytes over the time (achieved mask bytes/s) and that time at the 6.29 TB/s a float4 copy reaches.

The pipeline: TilePipeline images/s on the c2 shape (8 x 1024^2 tiles per step, 32 boxes each, rle=True) with overlap "order",
"logit" and "smallest", arms alternating, `--reps` runs each after an unmeasured first run.
usage: overlap_bench.py [--calls 20] [--steps 12] [--reps 2] [--model vit_h] [--kernels-only | --pipeline-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import samrs_amd  # noqa: E402
from samrs_amd import driver, synth  # noqa: E402

BATCH, BOXES = 8, 32
HBM_COPY_TBS = 6.29            # measured float4 copy rate of the part (8.0 TB/s spec)


def decoded_masks(n: int):
    """(engine, masks uint8 [n, 1024, 1024], low fp32 [n, 1, 256, 256], boxes) of n seeded boxes on one seeded tile."""
    sd = synth.make_state_dict(synth.CONFIGS["vit_tiny"], 0, logit_scale=synth.MARGIN_LOGIT_SCALE)
    sam = samrs_amd.sam_model_registry["vit_tiny"](state_dict=sd, precision="f16", max_images=1, max_prompts=64).to("cuda")
    pred = samrs_amd.SamPredictor(sam)
    img = synth.make_image(0)
    boxes, _ = synth.make_boxes(7, n)
    pred.set_image(img)
    tb = pred.transform.apply_boxes_torch(torch.from_numpy(boxes).cuda(), img.shape[:2])
    masks, _, low = pred.predict_torch(None, None, tb, None, multimask_output=False)
    return sam, masks[:, 0].contiguous().view(torch.uint8), low.contiguous(), boxes


def clip_to_boxes(masks: torch.Tensor, boxes: np.ndarray) -> torch.Tensor:
    n, h, w = masks.shape
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    b = torch.from_numpy(boxes).cuda()
    inside = (xx[None] >= b[:, 0, None, None]) & (xx[None] <= b[:, 2, None, None]) & (yy[None] >= b[:, 1, None, None]) & \
             (yy[None] <= b[:, 3, None, None])
    return (masks * inside.to(torch.uint8)).contiguous()


def timed(fn, before=None) -> float:
    if before is not None:
        before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernels(a) -> None:
    for n in (32, 64):
        sam, decoded, low, boxes = decoded_masks(n)
        eng = sam.engine
        h, w = decoded.shape[1:]
        labels = (torch.arange(n, dtype=torch.int32, device="cuda") % 18).to(torch.int32)
        ranks = torch.arange(n, dtype=torch.int32, device="cuda")
        seg = torch.empty(h, w, dtype=torch.uint8, device="cuda")
        order = torch.full((h, w), -1, dtype=torch.int32, device="cuda")
        pix, ins = (torch.zeros(18, dtype=torch.int64, device="cuda") for _ in range(2))
        removed = torch.zeros(n, dtype=torch.int64, device="cuda")
        for name, src in (("decoded", decoded), ("boxed", clip_to_boxes(decoded, boxes))):
            work = src.clone()
            contested = float(((src != 0).sum(0) >= 2).float().mean())
            arms = {
                "samrs_paint": (lambda: eng.paint(work, labels, seg, pix, ins), lambda: work.copy_(src), n * h * w + h * w),
                "samrs_scene_claim": (lambda: eng.scene_claim(work, ranks, (0, 0, w, h), order, labels, pix, ins), lambda: work.copy_(src),
                                      n * h * w + 8 * h * w),
                "samrs_resolve_overlaps": (lambda: eng.resolve_overlaps(work, "logit", low=low, input_size=(h, w), owner_out=False,
                                                                        before_out=False, removed_out=removed),
                                           lambda: work.copy_(src), n * h * w),
            }
            ms = {k: [] for k in arms}
            for k, (fn, before, _) in arms.items():                      # unmeasured first call per arm
                timed(fn, before)
            work.copy_(src)
            for _ in range(a.calls):
                for k, (fn, before, _) in arms.items():
                    ms[k].append(timed(fn, before))
            work.copy_(src)
            for k, (_, _, nbytes) in arms.items():
                med = float(np.median(ms[k]))
                print(json.dumps({"kernel": k, "masks": n, "tile": [h, w], "set": name, "contested_share": round(contested, 4),
                                  "us_per_call_median": round(1e3 * med, 2), "us_per_call_min": round(1e3 * min(ms[k]), 2),
                                  "mask_bytes": n * h * w, "mask_tbytes_per_s": round(n * h * w / (med * 1e-3) / 1e12, 3),
                                  "bytes_to_move": nbytes, "us_at_hbm_copy_rate": round(nbytes / (HBM_COPY_TBS * 1e12) * 1e6, 2),
                                  "removed_pixels": int(removed.sum()) if k == "samrs_resolve_overlaps" else None}), flush=True)
        eng.close()


def items(n):
    base = [synth.make_image(i) for i in range(8)]
    out = []
    for i in range(n):
        b, l = synth.make_boxes(i, BOXES)
        out.append(driver.WorkItem(f"T{i:05d}", base[i % 8], b, l))
    return out


def run_arm(sam, work, overlap):
    pipe = driver.TilePipeline(sam, 18, batch=BATCH, box_batch=BOXES, max_boxes=BOXES, rle=True, overlap=overlap)
    removed = [0]

    def sink(res, rel):
        removed[0] += sum(int(r.removed.sum()) for r in res if r.removed is not None)
        rel()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = pipe.run(driver.batched(work, BATCH), sink)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"pipeline": "TilePipeline", "overlap": overlap, "images": n, "images_per_s": round(n / dt, 1), "seconds": round(dt, 3),
            "removed_pixels_per_image": removed[0] // max(n, 1)}


def pipeline(a) -> None:
    sd = synth.make_state_dict(synth.CONFIGS[a.model], 0, logit_scale=synth.MARGIN_LOGIT_SCALE)
    sam = samrs_amd.sam_model_registry[a.model](state_dict=sd, precision="f16", max_images=2 * BATCH, max_prompts=64, max_points=1).to("cuda")
    work = items(a.steps * BATCH)
    arms = ("order", "logit", "smallest")
    for arm in arms:
        run_arm(sam, work[:3 * BATCH], arm)                               # unmeasured first run per arm
    for rep in range(a.reps):
        for arm in arms:
            r = run_arm(sam, work, arm)
            r["rep"], r["model"] = rep, a.model
            print(json.dumps(r), flush=True)
    sam.engine.close()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--pipeline-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("overlap_bench.py measures on the GPU: no HIP device found")
    if not a.pipeline_only:
        kernels(a)
    if not a.kernels_only:
        pipeline(a)


if __name__ == "__main__":
    main()
