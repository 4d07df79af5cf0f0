#!/usr/bin/env python3
"""What TilePipeline(polygons=True) costs on the c2 shape (ViT-H, 8 x 1024^2 tiles per step, 32 boxes each, rle=True): the option
off and on, arms alternating in one process, one JSON line per run with images/s of the loop and the decoder stream's time per
step (hipEvents on the decoder stream around each batch's decode, after its wait for the encoder).  The masks of a random-init model
are noise (about 10^5 .. 10^6 crack edges each), so the on arm runs with --max-edges 2^21 (every mask is traced: the worst case) and
once more with the default cap of 65536 (every mask is over the cap: the floor -- edge masks and one scan per mask, no ranking).
Then samrs_mask_polygons alone: ms per call on 32 masks of 1024^2, for the masks this (random-init) model paints, for blob-shaped
masks (an ellipse with 1 % pin-holes and 0.3 % speckle, the shape a trained model's masks have) and for clean ellipses, one JSON line
each, the first masks of each kind checked against tests/polygon_ref.py once.
usage: polygons_bench.py [--steps 24] [--reps 2] [--model vit_h] [--warm 3] [--standalone-only] [--out profiles/polygons_bench.txt]
(`rocprofv3 --kernel-trace --stats -- python tools/polygons_bench.py --standalone-only`, a run of its own, gives the time per kernel:
pg_double_kernel is the ranking rounds)"""
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
import polygon_ref  # noqa: E402  (tests/polygon_ref.py: the host restatement)
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


ALL_EDGES = 1 << 21            # no 1024^2 mask has more crack edges


def run_arm(sam, work, on, max_edges=ALL_EDGES):
    kw = dict(polygons=True, polygon_buffer_mb=1024, polygon_max_edges=max_edges) if on else {}
    pipe = driver.TilePipeline(sam, 18, batch=BATCH, box_batch=BOXES, max_boxes=BOXES, rle=True, **kw)
    stats = [0, 0, 0]              # masks traced, masks over the cap, vertices

    def sink(res, rel):
        for r in res:
            if r.polygon_table is not None:
                t = r.polygon_table
                stats[0] += int((t[:, 1] >= 0).sum())
                stats[1] += int((t[:, 1] == -1).sum())
                stats[2] += int(t[t[:, 3] > 0, 3].sum())
        rel()

    events = time_decode(pipe)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = pipe.run(driver.batched(work, BATCH), sink)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dec = decode_ms(events)
    name = "polygons_off" if not on else ("polygons_on" if max_edges == ALL_EDGES else f"polygons_on_cap_{max_edges}")
    return {"arm": name, "images": n, "images_per_s": round(n / dt, 1),
            "decode_ms_per_step": round(sum(dec) / len(dec), 3), "decode_ms_per_step_min": round(min(dec), 3),
            "masks_traced": stats[0], "masks_over_cap": stats[1], "vertices": stats[2]}


def standalone(sam, name, masks, max_edges, reps=10, check=2):
    eng = sam.engine
    n, h, w = masks.shape
    v = torch.empty(n * min(max_edges, 2 * h * w + 4), 2, dtype=torch.int32, device="cuda")
    r = torch.empty(v.shape[0] // 4, 4, dtype=torch.int32, device="cuda")
    cur = torch.zeros(2, dtype=torch.int64, device="cuda")
    tab = torch.empty(n, 5, dtype=torch.int64, device="cuda")
    ms = []
    for _ in range(reps + 2):
        cur.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.mask_polygons(masks, (0, 0), max_edges, v, r, cur, tab)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    host = masks[:check].cpu().numpy()
    wv, wr, wc, wt = polygon_ref.mask_polygons(list(host), max_edges=max_edges)
    t_ = tab.cpu().numpy()
    exact = (t_[:check].tolist() == wt.tolist() and np.array_equal(v[:wc[0]].cpu().numpy(), wv) and np.array_equal(r[:wc[1]].cpu().numpy(), wr))
    t = sorted(ms[-reps:])
    emit({"standalone": name, "masks": n, "side": w, "max_edges": max_edges, "ms_per_call_median": round(t[len(t) // 2], 4),
          "ms_per_call_min": round(t[0], 4), "edges_mean": round(float(t_[:, 4].mean()), 1), "rings_mean": round(float(t_[:, 1].mean()), 1),
          "vertices_mean": round(float(t_[:, 3].mean()), 1), "masks_checked": check, "equals_polygon_ref": bool(exact)})


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--warm", type=int, default=3, help="steps of an unmeasured first run per arm")
    ap.add_argument("--standalone-only", action="store_true", help="skip the pipeline arms")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file (profiles/polygons_bench.txt)")
    a = ap.parse_args()
    sd = synth.make_state_dict(synth.CONFIGS[a.model], 0)
    sam = samrs_amd.sam_model_registry[a.model](state_dict=sd, precision="f16", max_images=2 * BATCH, max_prompts=64,
                                                max_points=1).to("cuda")
    emit({"tool": "polygons_bench", "model": a.model, "device": torch.cuda.get_device_name(0), "batch": BATCH, "boxes": BOXES,
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
        r = run_arm(sam, work, True, 65536)                        # the default cap: every mask of this model is over it
        r["rep"] = 0
        emit(r)
    # the call alone: the masks this model paints for one tile's 32 boxes, 32 blobs with speckle, 32 clean ellipses
    pred = samrs_amd.SamPredictor(sam)
    pred.set_image(synth.make_image(0))
    b, _ = synth.make_boxes(0, BOXES)
    tb = pred.transform.apply_boxes_torch(torch.from_numpy(b).cuda(), (1024, 1024))
    masks, _, _ = pred.predict_torch(None, None, tb, None, multimask_output=False)
    standalone(sam, "decoder_masks_random_init", masks[:, 0].view(torch.uint8).contiguous(), ALL_EDGES, check=1)
    standalone(sam, "blob_with_speckle", torch.from_numpy(np.stack([speckled_ellipse(i) for i in range(BOXES)])).cuda(), 65536)
    standalone(sam, "clean_ellipse", torch.from_numpy(np.stack([polygon_ref.ellipse(1024, 200 + 5 * i, 330 - 4 * i)
                                                                for i in range(BOXES)])).cuda(), 65536)
    sam.engine.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
