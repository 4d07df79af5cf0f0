#!/usr/bin/env python3
"""What TilePipeline(mask_boxes=True) costs on the c2 shape (ViT-H, 8 x 1024^2 tiles per step, 32 boxes each, rle=True): the option
off and on, arms alternating in one process, one JSON line per run with images/s of the loop and the decoder stream's time per
step (hipEvents on the decoder stream around each batch's decode, after its wait for the encoder).
Then samrs_mask_boxes alone: ms per call on 32 masks of 1024^2, for the masks this (random-init) model paints and for blob-shaped
masks (an ellipse with 1 % pin-holes and 0.3 % speckle, the shape a trained model's masks have), one JSON line each, checked
against tests/box_ref.py once.
usage: mask_boxes_bench.py [--steps 24] [--reps 2] [--model vit_h] [--warm 3] [--standalone-only] [--out profiles/mask_boxes_bench.txt]
(`rocprofv3 --kernel-trace --stats -- python tools/mask_boxes_bench.py --standalone-only`, a run of its own, gives the time per kernel)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import samrs_amd  # noqa: E402
from samrs_amd import driver, synth  # noqa: E402
from decode_timer import decode_ms, time_decode  # noqa: E402
import box_ref  # noqa: E402  (tests/box_ref.py: the host restatement)
from region_ref import speckled_ellipse  # noqa: E402  (tests/region_ref.py: the blob-with-speckle recipe of the tests)

BATCH, BOXES = 8, 32
LINES = []


def emit(rec: dict) -> None:
    line = json.dumps(rec)
    LINES.append(line)
    print(line, flush=True)


def items(n):
    base = [synth.make_image(i) for i in range(8)]
    out = []
    for i in range(n):
        b, l = synth.make_boxes(i, BOXES)
        out.append(driver.WorkItem(f"T{i:05d}", base[i % 8], b, l))
    return out


def run_arm(sam, work, on):
    pipe = driver.TilePipeline(sam, 18, batch=BATCH, box_batch=BOXES, max_boxes=BOXES, rle=True, mask_boxes=on)
    nonempty = [0]

    def sink(res, rel):
        for r in res:
            if r.mask_record is not None:
                nonempty[0] += int((r.mask_record[:, 6] > 0).sum())
        rel()

    events = time_decode(pipe)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = pipe.run(driver.batched(work, BATCH), sink)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dec = decode_ms(events)
    return {"arm": "boxes_on" if on else "boxes_off", "images": n, "images_per_s": round(n / dt, 1),
            "decode_ms_per_step": round(sum(dec) / len(dec), 3), "decode_ms_per_step_min": round(min(dec), 3),
            "non_empty_masks": nonempty[0]}


def standalone(sam, name, masks, reps=10):
    eng = sam.engine
    n, h, w = masks.shape
    hb = torch.empty(n, 4, dtype=torch.int32, device="cuda")
    rb = torch.empty(n, 4, 2, dtype=torch.float32, device="cuda")
    rec = torch.empty(n, 8, dtype=torch.int64, device="cuda")
    ms = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.mask_boxes(masks, (0, 0), hb, rb, rec)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    want = box_ref.mask_boxes(masks.cpu().numpy())
    exact = all(g.cpu().numpy().tobytes() == w_.tobytes() for g, w_ in zip((hb, rb, rec), want))
    t = sorted(ms[-reps:])
    emit({"standalone": name, "masks": n, "side": w, "mask_bytes": n * h * w, "ms_per_call_median": round(t[len(t) // 2], 4),
          "ms_per_call_min": round(t[0], 4), "hull_vertices_mean": round(float(rec[:, 6].double().mean()), 1),
          "non_empty_rows_mean": round(float((masks.view(n, h, w).amax(2) > 0).sum(1).double().mean()), 1), "equals_box_ref": bool(exact)})


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--warm", type=int, default=3, help="steps of an unmeasured first run per arm")
    ap.add_argument("--standalone-only", action="store_true", help="skip the pipeline arms")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file (profiles/mask_boxes_bench.txt)")
    a = ap.parse_args()
    sd = synth.make_state_dict(synth.CONFIGS[a.model], 0)
    sam = samrs_amd.sam_model_registry[a.model](state_dict=sd, precision="f16", max_images=2 * BATCH, max_prompts=64,
                                                max_points=1).to("cuda")
    emit({"tool": "mask_boxes_bench", "model": a.model, "device": torch.cuda.get_device_name(0), "batch": BATCH, "boxes": BOXES,
          "steps": a.steps, "reps": a.reps})
    if not a.standalone_only:
        work = items(a.steps * BATCH)
        for arm in (False, True):
            run_arm(sam, work[:a.warm * BATCH], arm)
        for rep in range(a.reps):
            for arm in (False, True):
                r = run_arm(sam, work, arm)
                r["rep"] = rep
                emit(r)
    # the call alone: the masks this model paints for one tile's 32 boxes, and 32 blobs with speckle
    pred = samrs_amd.SamPredictor(sam)
    pred.set_image(synth.make_image(0))
    b, _ = synth.make_boxes(0, BOXES)
    tb = pred.transform.apply_boxes_torch(torch.from_numpy(b).cuda(), (1024, 1024))
    masks, _, _ = pred.predict_torch(None, None, tb, None, multimask_output=False)
    standalone(sam, "decoder_masks_random_init", masks[:, 0].view(torch.uint8).contiguous())
    standalone(sam, "blob_with_speckle", torch.from_numpy(np.stack([speckled_ellipse(i) for i in range(BOXES)])).cuda())
    sam.engine.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
