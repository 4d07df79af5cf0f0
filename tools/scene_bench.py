#!/usr/bin/env python3
"""Scene mode against the tile loop fed the same windows, arms alternating in one call, two runs per arm, one JSON line per run:
  arm "scene": ScenePipeline on seeded 4096^2 scenes with 256 boxes each, rle=True;
  (and one last "scene_stages" run with a host clock and a device synchronise per stage, to say where a scene's time goes);
  arm "tiles": TilePipeline (the loop as it was before scene mode) fed the SAME planned windows as separate WorkItems -- the
               window's crop as the image, its boxes shifted into the window -- so both arms encode and decode the same pixels
               and prompts; the tile arm produces per-window class maps and RLE, not the scene's.
--kernels-only: the three scene entry points alone (one 1024^2 window of 32 masks on a 4096^2 scene, `--calls` calls each, device
events), with the bytes each must move and that over the 6.29 TB/s a float4 copy reaches on this part -- the run to put under
`rocprofv3 --kernel-trace --stats`.
usage: scene_bench.py [--scenes 4] [--reps 2] [--model vit_h] [--side 4096] [--boxes 256] | --kernels-only [--calls 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import samrs_amd  # noqa: E402
from samrs_amd import driver, scene, synth  # noqa: E402

BATCH, BOX_BATCH = 8, 64
HBM_COPY_TBS = 6.29            # measured float4 copy rate of the part (8.0 TB/s spec)


def scenes(n, side, boxes):
    out = []
    for i in range(n):
        b, l = synth.make_boxes(300 + i, boxes, side, side)
        out.append(driver.WorkItem(f"S{i}", synth.make_noise_image(300 + i, side, side), b, l))
    return out


def window_items(work, window, overlap, context):
    """The tile arm's input: every planned window of every scene as a WorkItem of its own."""
    out = []
    for it in work:
        H, W = it.image.shape[:2]
        windows, window_of = scene.plan_scene(H, W, it.boxes, window, overlap, context)
        wo = np.asarray(window_of)
        for k, (x0, y0, w, h) in enumerate(windows):
            idx = np.nonzero(wo == k)[0]
            out.append(driver.WorkItem(f"{it.key}/w{k}", np.ascontiguousarray(it.image[y0:y0 + h, x0:x0 + w]),
                                       it.boxes[idx] - np.array([x0, y0, x0, y0], np.float32), it.labels[idx]))
    return out


def run_scene(sam, work, a, stages=False):
    pipe = scene.ScenePipeline(sam, 18, window=a.window, overlap=a.overlap, context=a.context, batch=BATCH, box_batch=BOX_BATCH, rle=True)
    if stages:                                    # attribution run: a synchronise closes every stage, so its rate is not a result
        pipe.stage_seconds = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = pipe.run(work, lambda res, rel: rel())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    r = {"arm": "scene_stages" if stages else "scene", "scenes": len(work), "windows": n, "windows_per_s": round(n / dt, 1),
         "seconds": round(dt, 3)}
    if stages:
        r["ms_per_scene"] = {k: round(1e3 * v / len(work), 2) for k, v in pipe.stage_seconds.items()}
    return r


def run_tiles(sam, tiles, n_scenes):
    pipe = driver.TilePipeline(sam, 18, batch=BATCH, box_batch=BOX_BATCH, max_boxes=max(len(t.labels) for t in tiles), rle=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = pipe.run(driver.batched(tiles, BATCH), lambda res, rel: rel())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"arm": "tiles", "scenes": n_scenes, "windows": n, "windows_per_s": round(n / dt, 1), "seconds": round(dt, 3)}


def kernels_only(a):
    sam = samrs_amd.sam_model_registry["vit_tiny"](max_images=1, max_prompts=4).to("cuda")
    eng = sam.engine
    H = W = a.side
    n, h, w, x0, y0 = 32, 1024, 1024, 1536, 768
    g = torch.Generator(device="cuda").manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda"), torch.arange(w, device="cuda"), indexing="ij")
    cx, cy = torch.rand(n, generator=g, device="cuda") * w, torch.rand(n, generator=g, device="cuda") * h
    r = 20 + torch.rand(n, generator=g, device="cuda") * 200
    masks = (((xx[None] - cx[:, None, None]) ** 2 + (yy[None] - cy[:, None, None]) ** 2) < (r * r)[:, None, None]).to(torch.uint8)
    ranks = torch.arange(n, dtype=torch.int32, device="cuda")
    labels = (ranks % 18).to(torch.int32)
    order = torch.full((H, W), -1, dtype=torch.int32, device="cuda")
    seg = torch.empty(H, W, dtype=torch.uint8, device="cuda")
    pix, ins = (torch.zeros(18, dtype=torch.int64, device="cuda") for _ in range(2))
    out = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    cur = torch.zeros(1, dtype=torch.int64, device="cuda")
    tab = torch.zeros(n, 3, dtype=torch.int64, device="cuda")
    win = (x0, y0, w, h)
    calls = {
        "scene_claim": (lambda: eng.scene_claim(masks, ranks, win, order, labels, pix, ins), n * h * w + 2 * 4 * h * w),
        "scene_resolve": (lambda: eng.scene_resolve(order, labels, seg), 5 * H * W),
        # bit-pack reads the masks and writes (w + 1) ceil(H / 32) words per mask; the run tables that follow depend on the masks
        "rle_encode_placed": (lambda: (cur.zero_(), eng.rle_encode_placed(masks, win, (H, W), out, cur, tab)), n * (h * w + (w + 1) * ((H + 31) // 32) * 4)),
    }
    for name, (fn, nbytes) in calls.items():
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        print(json.dumps({"standalone": name, "masks": n, "window": [w, h], "scene": [H, W], "ms_per_call_median": round(float(np.median(ms)), 4),
                          "ms_per_call_min": round(min(ms), 4), "bytes_to_move": nbytes,
                          "us_at_hbm_copy_rate": round(nbytes / (HBM_COPY_TBS * 1e12) * 1e6, 2)}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=4)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--boxes", type=int, default=256)
    ap.add_argument("--window", type=int, default=1024)
    ap.add_argument("--overlap", type=int, default=256)
    ap.add_argument("--context", type=float, default=2.0)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only(a)
        return
    sd = synth.make_state_dict(synth.CONFIGS[a.model], 0)
    sam = samrs_amd.sam_model_registry[a.model](state_dict=sd, precision="f16", max_images=2 * BATCH, max_prompts=BOX_BATCH,
                                                max_points=1).to("cuda")
    work = scenes(a.scenes, a.side, a.boxes)
    tiles = window_items(work, a.window, a.overlap, a.context)
    run_scene(sam, work[:1], a)                                       # unmeasured first run per arm
    run_tiles(sam, tiles[:2 * BATCH], 1)
    for rep in range(a.reps):
        for arm in ("tiles", "scene"):
            r = run_tiles(sam, tiles, len(work)) if arm == "tiles" else run_scene(sam, work, a)
            r["rep"] = rep
            print(json.dumps(r), flush=True)
    print(json.dumps(run_scene(sam, work, a, stages=True)), flush=True)
    sam.engine.close()


if __name__ == "__main__":
    main()
