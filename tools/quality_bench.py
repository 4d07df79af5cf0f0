#!/usr/bin/env python3
"""What TilePipeline(quality=True) costs on bench.py's c2 loop (ViT-H, 8 x 1024^2 device-resident noise tiles per step from a pool of
64, 32 boxes each in one predict, no RLE: the pipeline `python bench.py` times, so the "off" arm is that number): three arms
alternating in one process -- quality off / on (scores only) / on with all three thresholds (scores + the gate) -- on the same
seeded tiles.  One JSON line per run: images/s of the loop and the decoder stream's time per step (hipEvents around each batch's
decode, after its wait for the encoder), then one summary line with the "on" and "thresholds" arms' cost as a fraction of the "off"
arm's step time and the off arm's own run-to-run spread.  The off arm is the loop `python bench.py` times.
usage: quality_bench.py [--steps 24] [--reps 3] [--model vit_h] [--warm 3] [--out profiles/quality_bench.txt]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import samrs_amd  # noqa: E402
from samrs_amd import driver, synth  # noqa: E402
from decode_timer import decode_ms, time_decode  # noqa: E402

BATCH, BOXES = 8, 32
ARMS = {"off": {}, "on": {"quality": True},
        "thresholds": {"min_stability": 0.5, "min_pred_iou": 0.05, "min_inside_box": 0.25}}


def items(n, pool=64):
    base = torch.stack([torch.from_numpy(synth.make_noise_image(i)) for i in range(pool)]).cuda()
    out = []
    for i in range(n):
        b, l = synth.make_boxes(i, BOXES)
        out.append(driver.WorkItem(i, base[i % pool], b, l))
    return out


def run_arm(sam, work, arm):
    pipe = driver.TilePipeline(sam, 18, batch=BATCH, box_batch=BOXES, max_boxes=BOXES, device_inputs=True, rle_buffer_mb=512, **ARMS[arm])
    dropped = [0]

    def sink(res, rel):
        for r in res:
            if r.kept is not None:
                dropped[0] += int((~r.kept).sum())
        rel()

    events = time_decode(pipe)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = pipe.run(driver.batched(work, BATCH), sink)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dec = decode_ms(events)
    return {"arm": arm, "images": n, "images_per_s": round(n / dt, 2), "step_ms": round(1e3 * dt * BATCH / n, 3),
            "decode_ms_per_step": round(sum(dec) / len(dec), 3), "decode_ms_per_step_min": round(min(dec), 3),
            "dropped": dropped[0]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--warm", type=int, default=3, help="steps of an unmeasured first run per arm")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "quality_bench.txt"),
                    help="the JSON lines are also saved to this file (default profiles/quality_bench.txt; '' = print only)")
    a = ap.parse_args()
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    sd = synth.make_state_dict(synth.CONFIGS[a.model], 0)
    work = items(a.steps * BATCH)
    sam = samrs_amd.sam_model_registry[a.model](state_dict=sd, precision="f16", max_images=2 * BATCH, max_prompts=BOXES,
                                                max_points=1).to("cuda")
    emit({"tool": "quality_bench", "model": a.model, "device": torch.cuda.get_device_name(0), "batch": BATCH, "boxes": BOXES,
          "steps": a.steps, "reps": a.reps, "arms": ARMS})
    for arm in ARMS:
        run_arm(sam, work[:a.warm * BATCH], arm)
    runs = {arm: [] for arm in ARMS}
    for rep in range(a.reps):
        for arm in ARMS:
            r = run_arm(sam, work, arm)
            r["rep"] = rep
            runs[arm].append(r)
            emit(r)
    mean = {arm: sum(r["step_ms"] for r in rs) / len(rs) for arm, rs in runs.items()}
    dec = {arm: sum(r["decode_ms_per_step"] for r in rs) / len(rs) for arm, rs in runs.items()}
    off = [r["images_per_s"] for r in runs["off"]]
    emit({"summary": True, "off_images_per_s_mean": round(sum(off) / len(off), 2), "off_images_per_s_min": min(off),
          "off_images_per_s_max": max(off), "off_spread_fraction": round((max(off) - min(off)) / (sum(off) / len(off)), 4),
          "step_ms_mean": {k: round(v, 3) for k, v in mean.items()},
          "decode_ms_per_step_mean": {k: round(v, 3) for k, v in dec.items()},
          "on_cost_fraction_of_off_step": round(mean["on"] / mean["off"] - 1.0, 4),
          "thresholds_cost_fraction_of_off_step": round(mean["thresholds"] / mean["off"] - 1.0, 4),
          "on_decode_cost_ms_per_step": round(dec["on"] - dec["off"], 3),
          "on_decode_cost_fraction_of_off_step": round((dec["on"] - dec["off"]) / mean["off"], 4)})
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sam.engine.close()


if __name__ == "__main__":
    main()
