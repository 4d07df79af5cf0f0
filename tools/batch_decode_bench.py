#!/usr/bin/env python3
"""TilePipeline with and without batch_decode on the same seeded tiles (the c2 shape: ViT-H, 8 x 1024^2 tiles per step, 32 boxes
each), arms alternating, at max_prompts 64 and 256: one JSON line per run with images/s of the loop, the decoder stream's time per
step (hipEvents on the decoder stream around each batch's decode, after its wait for the encoder) and max_prompts.
usage: batch_decode_bench.py [--steps 24] [--reps 2] [--model vit_h] [--max-prompts 64,256] [--warm 3]"""
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


def items(n):
    base = [synth.make_image(i) for i in range(8)]
    out = []
    for i in range(n):
        b, l = synth.make_boxes(i, BOXES)
        out.append(driver.WorkItem(f"T{i:05d}", base[i % 8], b, l))
    return out


def run_arm(sam, work, batch_decode):
    pipe = driver.TilePipeline(sam, 18, batch=BATCH, box_batch=BOXES, max_boxes=BOXES, rle=True, batch_decode=batch_decode)
    events = time_decode(pipe)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = pipe.run(driver.batched(work, BATCH), lambda res, rel: rel())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dec = decode_ms(events)
    return {"arm": "batch_decode" if batch_decode else "per_tile", "max_prompts": sam.max_prompts, "images": n,
            "images_per_s": round(n / dt, 1), "decode_ms_per_step": round(sum(dec) / len(dec), 3),
            "decode_ms_per_step_min": round(min(dec), 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--max-prompts", default="64,256")
    ap.add_argument("--warm", type=int, default=3, help="steps of an unmeasured first run per arm")
    a = ap.parse_args()
    sd = synth.make_state_dict(synth.CONFIGS[a.model], 0)
    work = items(a.steps * BATCH)
    for mp in (int(v) for v in a.max_prompts.split(",")):
        sam = samrs_amd.sam_model_registry[a.model](state_dict=sd, precision="f16", max_images=2 * BATCH, max_prompts=mp,
                                                    max_points=1).to("cuda")
        for arm in (False, True):
            run_arm(sam, work[:a.warm * BATCH], arm)
        for rep in range(a.reps):
            for arm in (False, True):
                r = run_arm(sam, work, arm)
                r["rep"] = rep
                print(json.dumps(r), flush=True)
        sam.engine.close()


if __name__ == "__main__":
    main()
