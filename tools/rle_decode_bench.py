#!/usr/bin/env python3
"""COCO RLE strings -> masks on the device, two ways on the same strings, arms alternating in one process, one JSON line per arm.

  device  rle.decode_device: pack the strings on the host, one upload, samrs_rle_decode; the masks stay on the device
  host    rle.decode per string (the Python loop over counts) + np.stack + upload: what coco_ap.evaluate_files did before
  kernels samrs_rle_decode alone on strings that are already on the device (device events): the share of `device` that is GPU work

Three mask kinds at 1024^2, 32 masks per call: "blob" (smooth blobs clipped to a box, what a box-prompted decoder returns: a few
thousand counts), "noise" (p = 0.5 per pixel: ~5 * 10^5 counts per mask, the multi-block scans) and "empty" (one count).  device and
host are wall-clock around work that ends in a device synchronise; every arm has an unmeasured first call.  Before timing, the
device result is compared with the host result, exactly.
usage: rle_decode_bench.py [--calls 5] [--noise-calls 2] [--masks 32]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import samrs_amd  # noqa: E402
from samrs_amd import rle  # noqa: E402

H = W = 1024


def blob_masks(n: int, seed: int) -> np.ndarray:
    """smooth blobs (a 16 x 16 seeded field, upsampled and thresholded) clipped to a seeded box each"""
    g = torch.Generator().manual_seed(seed)
    field = torch.nn.functional.interpolate(torch.randn(n, 1, 16, 16, generator=g), size=(H, W), mode="bicubic", align_corners=False)[:, 0]
    m = (field > 0.2).numpy()
    rng = np.random.default_rng(seed)
    for j in range(n):
        x0, y0 = rng.integers(0, W - 300, 2)
        bw, bh = rng.integers(100, 300, 2)
        keep = np.zeros((H, W), bool)
        keep[y0:y0 + bh, x0:x0 + bw] = True
        m[j] &= keep
    return m


def wall(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def events(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--noise-calls", type=int, default=2, help="timed calls of the noise kind (its host arm takes seconds per call)")
    ap.add_argument("--masks", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rle_decode_bench.py measures on the GPU: no HIP device found")
    sam = samrs_amd.sam_model_registry["vit_tiny"](max_prompts=1).to("cuda")
    eng = sam.engine
    n = a.masks
    kinds = {"blob": blob_masks(n, 1), "noise": np.random.default_rng(2).random((n, H, W)) < 0.5, "empty": np.zeros((n, H, W), bool)}
    for kind, masks in kinds.items():
        rles = [rle.encode(m) for m in masks]
        buf, table = rle.pack_strings(rles)
        dbuf, dtab = torch.from_numpy(buf).cuda(), torch.from_numpy(table).cuda()
        out = torch.empty(n, H, W, dtype=torch.uint8, device="cuda")
        area, status = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
        keep = {}
        arms = {
            "device": lambda: keep.__setitem__("device", rle.decode_device(eng, rles)),
            "host": lambda: keep.__setitem__("host", torch.from_numpy(np.stack([rle.decode(r) for r in rles]).view(np.uint8)).cuda()),
            "kernels": lambda: eng.rle_decode(dbuf, dtab, (H, W), out=out, areas_out=area, status_out=status),
        }
        timers = {"device": wall, "host": wall, "kernels": events}
        for k, fn in arms.items():                                          # unmeasured first call per arm
            timers[k](fn)
        want = torch.from_numpy(masks.view(np.uint8)).cuda()
        exact = bool(torch.equal(keep["device"], want) and torch.equal(keep["host"], want) and torch.equal(out, want)
                     and int(status.abs().sum()) == 0)
        if not exact:
            raise SystemExit(f"{kind}: the arms do not agree with the masks that were encoded")
        ms = {k: [] for k in arms}
        for _ in range(a.noise_calls if kind == "noise" else a.calls):
            for k, fn in arms.items():
                ms[k].append(timers[k](fn))
        counts = int(sum(len(rle.string_to_counts(r["counts"])) for r in rles[:4]) / 4)
        for k in arms:
            med = float(np.median(ms[k]))
            print(json.dumps({"arm": k, "kind": kind, "masks": n, "tile": [H, W], "string_bytes": int(table[:, 1].sum()),
                              "counts_per_mask": counts, "calls": len(ms[k]), "ms_per_call_median": round(med, 3),
                              "ms_per_call_min": round(min(ms[k]), 3), "clock": "device events" if k == "kernels" else "host, synchronised",
                              "mask_gbytes_per_s": round(n * H * W / (med * 1e-3) / 1e9, 2), "exact": exact}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
