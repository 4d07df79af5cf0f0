#!/usr/bin/env python3
"""What samrs_fill_polygons costs, and what TilePipeline(polygon_iou=True) adds to the loop.  One JSON line:
  (a) "fill": Engine.fill_polygons on 32 masks of 1024^2 -- blobs with pin-holes and speckle (tests/region_ref.py's recipe) --, for the
      rings Engine.mask_polygons traced and for the same rings after Engine.simplify_polygons at 1 px, each with a mask output
      (masks_out + ref + counts) and counts only (masks_out NULL: what the pipeline option runs); four arms alternating, three passes,
      ms per call from hipEvents (median of the passes' medians, and the minimum);
  (b) "host": polygons.rasterize_any for the same rings, ms per mask over the first --check masks, whose device fill is compared with it;
  (c) "pipeline": TilePipeline on the c2 shape (8 x 1024^2 tiles per step, 32 boxes each, rle=True) with polygons=True and
      polygon_epsilon=1.0, polygon_iou off and on, arms alternating in one process: images/s of the loop and the decoder stream's ms
      per step.  A random-init model's masks are noise (about 3 10^5 crack edges each): with --max-edges 2^21 (default) every mask is
      traced, simplified and filled -- the worst case for all three stages; 65536 leaves every such mask untraced (the floor);
  (d) "stages": where (c)'s difference goes -- one chunk of that loop alone (the 32 masks this model paints for one tile, buffers of the
      loop's capacity): ms per call of mask_polygons, of mask_polygons + simplify_polygons at 1 px, and of the counts-only fill of the
      traced and of the simplified rings.  With the option on, the loop simplifies once per chunk instead of once per batch.
No pass mark is set.
usage: polygon_fill_bench.py [--reps 10] [--check 2] [--model vit_h] [--steps 12] [--warm 2] [--max-edges E] [--no-pipeline]
                             [--out profiles/polygon_fill_bench.txt]"""
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
from samrs_amd import driver, polygons, synth  # noqa: E402
from decode_timer import decode_ms, time_decode  # noqa: E402
from region_ref import speckled_ellipse  # noqa: E402

N, SIDE, BATCH, BOXES = 32, 1024, 8, 32


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
    return t[len(t) // 2], t[0]


def traced(eng, masks, eps):
    v, r, c, t = eng.mask_polygons(masks, (0, 0), 1 << 18)
    if eps:
        eng.simplify_polygons(t, r, v, c, eps)
    torch.cuda.synchronize()
    assert (t[:, 1] >= 0).all(), "a mask was not traced"
    return t, r, v


def fill_arms(eng, reps, check):
    host = np.stack([speckled_ellipse(i) for i in range(N)])
    masks = torch.from_numpy(host).cuda()
    out = torch.empty(N, SIDE, SIDE, dtype=torch.uint8, device="cuda")
    counts = torch.empty(N, 3, dtype=torch.int64, device="cuda")
    sets = {"traced": traced(eng, masks, 0.0), "simplified_1px": traced(eng, masks, 1.0)}
    arms = {}
    for name, (t, r, v) in sets.items():
        arms[name + "_masks"] = lambda t=t, r=r, v=v: eng.fill_polygons(t, r, v, (SIDE, SIDE), out=out, ref=masks, counts_out=counts)
        arms[name + "_counts_only"] = lambda t=t, r=r, v=v: eng.fill_polygons(t, r, v, (SIDE, SIDE), out=False, ref=masks, counts_out=counts)
    times = {a: [] for a in arms}
    for _ in range(3):
        for a, fn in arms.items():
            times[a].append(timed(fn, reps))
    rec = {a: {"ms_per_call_median": round(sorted(m for m, _ in ts)[1], 4), "ms_per_call_min": round(min(m for _, m in ts), 4)}
           for a, ts in times.items()}
    hosts = {}
    for name, (t, r, v) in sets.items():
        tn, rn, vn = (x.cpu().numpy() for x in (t, r, v))
        m, c = eng.fill_polygons(t, r, v, (SIDE, SIDE), ref=masks)
        m, c = m.cpu().numpy(), c.cpu().numpy()
        w0, same = time.perf_counter(), True
        for j in range(check):
            same = same and np.array_equal(polygons.rasterize_any(polygons.rings_of(tn, rn, vn, j), SIDE, SIDE), m[j])
        iou = polygons.iou_from_counts(c)
        hosts[name] = {"rasterize_any_ms_per_mask": round(1e3 * (time.perf_counter() - w0) / max(check, 1), 2), "masks_checked": check,
                       "device_equals_rasterize_any": bool(same), "vertices": int(tn[:, 3].sum()), "rings": int(tn[:, 1].sum()),
                       "iou_mean": round(float(iou.mean()), 6), "iou_min": round(float(iou.min()), 6)}
    return rec, hosts


def stage_arms(sam, max_edges):
    eng = sam.engine
    pred = samrs_amd.SamPredictor(sam)
    pred.set_image(synth.make_image(0))
    b, _ = synth.make_boxes(0, BOXES)
    tb = pred.transform.apply_boxes_torch(torch.from_numpy(b).cuda(), (SIDE, SIDE))
    masks, _, _ = pred.predict_torch(None, None, tb, None, multimask_output=False)
    masks = masks[:, 0].view(torch.uint8).contiguous()
    nv = (1024 << 20) // 12                                         # polygon_buffer_mb=1024, as run_arm
    v = torch.empty(nv, 2, dtype=torch.int32, device="cuda")
    r = torch.empty(nv // 4, 4, dtype=torch.int32, device="cuda")
    cur, tab = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.empty(BOXES, 5, dtype=torch.int64, device="cuda")
    cnt = torch.empty(BOXES, 3, dtype=torch.int64, device="cuda")

    def trace():
        cur.zero_()
        eng.mask_polygons(masks, (0, 0), max_edges, v, r, cur, tab)

    def trace_simplify():
        trace()
        eng.simplify_polygons(tab, r, v, cur, 1.0)

    def fill():
        eng.fill_polygons(tab, r, v, (SIDE, SIDE), out=False, ref=masks, counts_out=cnt)

    rec = {"masks": BOXES, "trace_ms": round(timed(trace, 5)[0], 3), "trace_simplify_ms": round(timed(trace_simplify, 5)[0], 3)}
    trace()
    rec["fill_counts_traced_ms"] = round(timed(fill, 5)[0], 3)
    t0 = tab.cpu().numpy()
    rec.update(masks_traced=int((t0[:, 1] >= 0).sum()), vertices_traced=int(t0[t0[:, 3] > 0, 3].sum()))
    trace_simplify()
    rec["fill_counts_simplified_ms"] = round(timed(fill, 5)[0], 3)
    t1 = tab.cpu().numpy()
    rec["vertices_simplified"] = int(t1[t1[:, 3] > 0, 3].sum())
    return rec


def run_arm(sam, work, on, max_edges):
    pipe = driver.TilePipeline(sam, 18, batch=BATCH, box_batch=BOXES, max_boxes=BOXES, rle=True, polygons=True, polygon_buffer_mb=1024,
                               polygon_max_edges=max_edges, polygon_epsilon=1.0, polygon_iou=on)
    stat = driver.PolygonIoUStat()

    def sink(res, rel):
        for r in res:
            if r.polygon_counts is not None:
                stat.add(r.polygon_counts)
        rel()

    events = time_decode(pipe)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = pipe.run(driver.batched(work, BATCH), sink)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dec = decode_ms(events)
    rec = {"images_per_s": round(n / dt, 1), "decode_ms_per_step": round(sum(dec) / len(dec), 3), "decode_ms_per_step_min": round(min(dec), 3)}
    if on:
        rec.update(instances_scored=stat.n, iou_average=round(stat.total / stat.n, 6) if stat.n else None)
    return rec


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--check", type=int, default=2, help="masks per ring set that are also filled on the host and compared")
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warm", type=int, default=2, help="steps of an unmeasured first run per pipeline arm")
    ap.add_argument("--max-edges", type=int, default=1 << 21, help="polygon_max_edges of the pipeline arms")
    ap.add_argument("--no-pipeline", action="store_true", help="(a) and (b) only: neither the loop nor its stages")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file (profiles/polygon_fill_bench.txt)")
    a = ap.parse_args()
    sd = synth.make_state_dict(synth.CONFIGS[a.model], 0)
    sam = samrs_amd.sam_model_registry[a.model](state_dict=sd, precision="f16", max_images=2 * BATCH, max_prompts=64, max_points=1).to("cuda")
    rec = {"tool": "polygon_fill_bench", "device": torch.cuda.get_device_name(0), "masks_per_call": N, "side": SIDE, "reps": a.reps}
    rec["fill"], rec["host"] = fill_arms(sam.engine, a.reps, a.check)
    if not a.no_pipeline:
        base = [synth.make_image(i) for i in range(8)]
        work = []
        for i in range(a.steps * BATCH):
            b, l = synth.make_boxes(i, BOXES)
            work.append(driver.WorkItem(f"T{i:05d}", base[i % 8], b, l))
        for on in (False, True):
            run_arm(sam, work[:a.warm * BATCH], on, a.max_edges)
        runs = {"polygon_iou_off": [], "polygon_iou_on": []}
        for _ in range(2):
            for on in (False, True):
                runs["polygon_iou_on" if on else "polygon_iou_off"].append(run_arm(sam, work, on, a.max_edges))
        rec["stages"] = stage_arms(sam, a.max_edges)
        rec["pipeline"] = dict(model=a.model, batch=BATCH, boxes=BOXES, steps=a.steps, polygon_epsilon=1.0, polygon_max_edges=a.max_edges, **runs)
    sam.engine.close()
    line = json.dumps(rec)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
