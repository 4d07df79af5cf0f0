#!/usr/bin/env python3
"""What samrs_simplify_polygons costs beside the tracing it follows, on annotation-shaped synthetic masks: 32 masks of 1024^2 per call
-- rotated bars (a 300 x 40 px "ship" at 30 degrees and its kin), rotated ellipses, and blobs with pin-holes and speckle
(tests/region_ref.py's recipe) --, arms alternating in one process:
  trace            Engine.mask_polygons alone: the parent commit's path;
  trace+simplify   the same call followed by Engine.simplify_polygons at epsilon 0.5, 1 and 2 pixels;
  host             the host statement (tests/polygon_simplify_ref.py) per mask, on the rings the device traced: the plain recursion over
                   Python ints and its numpy form -- the per-mask host loop the entry point replaces (cv2.approxPolyDP is not
                   installable here; nothing is pinned against it).
One JSON line per arm and kind of mask: ms per call (hipEvents around the call, median and minimum of --reps), vertices before and
after, and for the first --check masks the IoU of polygons.rasterize_any(simplified rings) against the mask and whether the device's
rings equal the host statement's.  The masks are synthetic shapes, the model's weights play no part: the IoU figures say something
about the geometry of the rule only, not about SAM's masks.  No pass mark is set.
usage: polygon_simplify_bench.py [--reps 10] [--check 2] [--model vit_tiny] [--out profiles/polygon_simplify_bench.txt]"""
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
from samrs_amd import polygons  # noqa: E402
import polygon_simplify_ref as ps_ref  # noqa: E402  (tests/: the host statement)
from region_ref import speckled_ellipse  # noqa: E402

N, SIDE = 32, 1024
EPSILONS = (0.5, 1.0, 2.0)
LINES = []


def emit(rec: dict) -> None:
    line = json.dumps(rec)
    LINES.append(line)
    print(line, flush=True)


def rotated(kind: str, i: int) -> np.ndarray:
    """a bar or an ellipse of about 300 x 40 .. 400 x 120 pixels at 30 + 11 i degrees around the tile's centre"""
    yy, xx = np.mgrid[0:SIDE, 0:SIDE].astype(np.float64)
    a = np.deg2rad(30.0 + 11.0 * i)
    u = (xx - 511.5) * np.cos(a) + (yy - 511.5) * np.sin(a)
    v = -(xx - 511.5) * np.sin(a) + (yy - 511.5) * np.cos(a)
    hu, hv = 150.0 + 3.0 * i, 20.0 + 1.5 * i
    if kind == "bar":
        return ((np.abs(u) <= hu) & (np.abs(v) <= hv)).astype(np.uint8)
    return ((u / hu) ** 2 + (v / hv) ** 2 <= 1.0).astype(np.uint8)


def timed(fn, reps):
    ms = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    t = sorted(ms[-reps:])
    return round(t[len(t) // 2], 4), round(t[0], 4)


def bench(eng, name: str, host: np.ndarray, reps: int, check: int) -> None:
    masks = torch.from_numpy(host).cuda()
    cap = 1 << 18
    v = torch.empty(N * cap // 4, 2, dtype=torch.int32, device="cuda")
    r = torch.empty(v.shape[0] // 4, 4, dtype=torch.int32, device="cuda")
    cur = torch.zeros(2, dtype=torch.int64, device="cuda")
    tab = torch.empty(N, 5, dtype=torch.int64, device="cuda")

    def trace():
        cur.zero_()
        eng.mask_polygons(masks, (0, 0), cap, v, r, cur, tab)

    def both(eps):
        trace()
        eng.simplify_polygons(tab, r, v, cur, eps)

    arms = [("trace", trace)] + [(f"trace+simplify eps={e}", (lambda e=e: both(e))) for e in EPSILONS]
    times = {a: [] for a, _ in arms}
    for _ in range(3):                                              # arms alternating: three passes over all of them
        for a, fn in arms:
            times[a].append(timed(fn, reps))
    trace()
    torch.cuda.synchronize()
    t0, r0, v0, c0 = (x.cpu().numpy().copy() for x in (tab, r, v[:int(cur[0])], cur))
    assert (t0[:, 1] >= 0).all(), "a mask was not traced or placed: raise the capacities"
    before = int(t0[:, 3].sum())
    for (a, fn), eps in zip(arms, (None,) + EPSILONS):
        med = sorted(m for m, _ in times[a])[1]
        rec = {"masks": name, "arm": a, "n": N, "side": SIDE, "ms_per_call_median": med, "ms_per_call_min": min(m for _, m in times[a]),
               "rings": int(t0[:, 1].sum()), "vertices_before": before}
        if eps is not None:
            fn()
            torch.cuda.synchronize()
            t1, r1, v1 = tab.cpu().numpy(), r.cpu().numpy(), v[:int(cur[0])].cpu().numpy()
            q = int(round(16 * eps))
            ious, same = [], True
            for j in range(check):
                got = polygons.rings_of(t1, r1, v1, j)
                want = [(p[ps_ref.simplify_ring_fast(p, q)], h) for p, h in polygons.rings_of(t0, r0, v0, j)]
                same = same and len(got) == len(want) and all(np.array_equal(g[0], w[0]) for g, w in zip(got, want))
                fill = polygons.rasterize_any(got, SIDE, SIDE)
                ious.append(float((fill & host[j]).sum()) / max(1.0, float((fill | host[j]).sum())))
            rec.update(vertices_after=int(t1[:, 3].sum()), masks_checked=check, equals_host_statement=bool(same),
                       iou_rasterize_any_min=round(min(ious), 5), iou_rasterize_any_mean=round(sum(ious) / len(ious), 5))
        emit(rec)
    # the host loop: per mask, on the traced rings (the plain recursion on the first `check` masks, its numpy form on all)
    for eps in EPSILONS:
        q = int(round(16 * eps))
        w0 = time.perf_counter()
        for j in range(check):
            for p, _ in polygons.rings_of(t0, r0, v0, j):
                ps_ref.simplify_ring(p, q)
        plain = (time.perf_counter() - w0) / check
        w0 = time.perf_counter()
        for j in range(N):
            for p, _ in polygons.rings_of(t0, r0, v0, j):
                ps_ref.simplify_ring_fast(p, q)
        fast = (time.perf_counter() - w0) / N
        emit({"masks": name, "arm": f"host eps={eps}", "ms_per_mask_plain_python": round(1e3 * plain, 3),
              "ms_per_mask_numpy": round(1e3 * fast, 3), "ms_per_call_of_32_numpy": round(32e3 * fast, 2)})


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--check", type=int, default=2, help="masks whose rings are compared with the host statement and rasterized")
    ap.add_argument("--model", default="vit_tiny", help="the engine that hosts the kernels (no weights are used)")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file (profiles/polygon_simplify_bench.txt)")
    a = ap.parse_args()
    sam = samrs_amd.sam_model_registry[a.model](max_images=1, max_prompts=4).to("cuda")
    emit({"tool": "polygon_simplify_bench", "device": torch.cuda.get_device_name(0), "masks_per_call": N, "side": SIDE, "reps": a.reps,
          "note": "synthetic shapes, no model weights involved: the IoU figures describe the geometry of the rule, not SAM's masks"})
    bench(sam.engine, "rotated_bars", np.stack([rotated("bar", i) for i in range(N)]), a.reps, a.check)
    bench(sam.engine, "rotated_ellipses", np.stack([rotated("ellipse", i) for i in range(N)]), a.reps, a.check)
    bench(sam.engine, "blob_with_speckle", np.stack([speckled_ellipse(i) for i in range(N)]), a.reps, a.check)
    sam.engine.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
