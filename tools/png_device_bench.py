#!/usr/bin/env python3
"""The generation CLI (samrs_amd.generate.run) with and without --png-device on the same seeded tiles, arms alternating: one JSON
line per run with images/s of the loop and the host thread time per image by stage.  Random weights paint noise-like class maps
(the worst case of the PNG encoders).  Thread pools are sized from this process's CPU share (run it under `taskset -c 0,1` for one
rank's share when eight ranks share 16 CPUs).
usage: png_device_bench.py [--tiles 320] [--model vit_h] [--reps 2] [--arms host,device] [--warm 16]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from samrs_amd import generate, synth, tile_io  # noqa: E402


def make_tiles(root: str, n: int):
    img_dir = os.path.join(root, "img")
    os.makedirs(img_dir)
    base = [synth.make_image(i) for i in range(8)]                      # 8 distinct tiles, re-used with a roll
    ann = {}
    for i in range(n):
        tile_io.write_rgb(os.path.join(img_dir, f"T{i:05d}.png"), np.ascontiguousarray(np.roll(base[i % 8], 37 * (i // 8), axis=1)), 1)
        b, l = synth.make_boxes(i, 32)
        ann[f"T{i:05d}"] = {"boxes": b.tolist(), "labels": l.tolist()}
    return img_dir, ann


def run_arm(root, img_dir, ann, n, model, png_device):
    boxes = os.path.join(root, f"boxes_{n}.json")
    with open(boxes, "w") as f:
        json.dump({k: ann[k] for k in sorted(ann)[:n]}, f)
    out_dir = os.path.join(root, "out")
    shutil.rmtree(out_dir, ignore_errors=True)
    ns = argparse.Namespace(images=img_dir, boxes=boxes, out=out_dir, model=model, checkpoint=None, precision="f16", classes=None,
                            n_classes=18, palette=None, box_batch=64, no_rle=False, batch=8, resume=False, timing=True,
                            png_device=png_device)
    t = generate.run(ns)["timing"]
    stages = {k: round(1e3 * v / t["images"], 2) for k, v in sorted(t["stage_thread_seconds"].items()) if not k.startswith("loop.")}
    return {"arm": "device" if png_device else "host", "images": t["images"], "images_per_s": round(t["images"] / t["loop_seconds"], 1),
            "host_ms_per_image": round(sum(stages.values()), 2), "stages_ms_per_image": stages,
            "cpus": len(os.sched_getaffinity(0)), "io_threads": list(generate.io_threads(png_device=png_device))}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=320)
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--arms", default="host,device")
    ap.add_argument("--warm", type=int, default=16, help="tiles of an unmeasured first run per arm (kernel load, allocator)")
    a = ap.parse_args()
    arms = [s == "device" for s in a.arms.split(",")]
    root = tempfile.mkdtemp(prefix="samrs_png_")
    try:
        img_dir, ann = make_tiles(root, a.tiles)
        if a.warm:
            for dev in arms:
                run_arm(root, img_dir, ann, a.warm, a.model, dev)
        for rep in range(a.reps):
            for dev in arms:
                r = run_arm(root, img_dir, ann, a.tiles, a.model, dev)
                r["rep"] = rep
                print(json.dumps(r), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
