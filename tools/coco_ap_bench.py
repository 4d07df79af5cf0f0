#!/usr/bin/env python3
"""The COCO AP evaluation end measured two ways, arms alternating in one process, one JSON line per result.

The kernels: pack (predictions from mask bytes, ground truth from a label image) + pair counts + matching for 64 x 64 and 256 x 256
masks of one 1024^2 tile -- seeded ellipses, the ground truths painted into a label image in one colour each, the predictions the
same ellipses shifted by a few pixels.  Device events around each stage and around the whole chain, `--calls` rounds after an
unmeasured first one.  Beside them, for comparison, the same counts as a dense torch matmul of the flattened masks (fp32 operands:
exact below 2^24 set pixels per pair), with and without the conversion of the mask bytes it needs.  Every line
carries the bytes the stage has to move and that time at the 6.29 TB/s a float4 copy reaches.

The pipeline: InstancePipeline images/s (8 x 1024^2 tiles per step, 32 rotated boxes each, gt=True, rle=True, the box prompt, single
mask) with ap off and on, arms alternating, `--reps` runs each after an unmeasured first run.
usage: coco_ap_bench.py [--calls 20] [--steps 12] [--reps 2] [--model vit_h] [--kernels-only | --pipeline-only]"""
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
SIDE = 1024


def ellipses(n: int, seed: int, shift: int = 0) -> torch.Tensor:
    """uint8 [n, SIDE, SIDE] on the device: n seeded ellipses (semi-axes 8..96), moved right and down by `shift` pixels."""
    rng = np.random.default_rng(seed)
    c = torch.from_numpy(rng.uniform(64, SIDE - 64, size=(n, 2)).astype(np.float32)).cuda() + shift
    r = torch.from_numpy(rng.uniform(8, 96, size=(n, 2)).astype(np.float32)).cuda()
    yy, xx = torch.meshgrid(torch.arange(SIDE, device="cuda", dtype=torch.float32),
                            torch.arange(SIDE, device="cuda", dtype=torch.float32), indexing="ij")
    out = torch.empty(n, SIDE, SIDE, dtype=torch.uint8, device="cuda")
    for j in range(n):
        out[j] = ((((yy - c[j, 0]) / r[j, 0]) ** 2 + ((xx - c[j, 1]) / r[j, 1]) ** 2) <= 1).to(torch.uint8)
    return out


def label_image(gt: torch.Tensor):
    """(label uint8 [SIDE, SIDE, 3], colors uint8 [n, 3]): instance j painted in colour (j % 251 + 1, j // 251 + 1, 7), later on top."""
    n = gt.shape[0]
    colors = torch.tensor([[j % 251 + 1, j // 251 + 1, 7] for j in range(n)], dtype=torch.uint8, device="cuda")
    label = torch.zeros(SIDE, SIDE, 3, dtype=torch.uint8, device="cuda")
    for j in range(n):
        label[gt[j] != 0] = colors[j]
    return label.contiguous(), colors


def timed(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def kernels(a) -> None:
    sam = samrs_amd.sam_model_registry["vit_tiny"](precision="f16", max_images=1, max_prompts=4).to("cuda")
    eng = sam.engine
    hw = SIDE * SIDE
    words = hw // 64
    for n in (64, 256):
        gt = ellipses(n, 11)
        pred = ellipses(n, 11, shift=3)
        label, colors = label_image(gt)
        pp = torch.empty(n, words, dtype=torch.int64, device="cuda")
        gp = torch.empty(n, words, dtype=torch.int64, device="cuda")
        inter = torch.empty(n, n, dtype=torch.int64, device="cuda")
        ad, ag = (torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(2))
        scores = torch.from_numpy(np.random.default_rng(3).random(n).astype(np.float32)).cuda()
        outs = eng.coco_match(inter, ad, ag, scores)               # allocates the five tables once
        half = [None, None]                                        # the masks as fp32 [n, hw]: 1 GiB each at n = 256

        def to_half():
            half[0], half[1] = pred.view(n, hw).to(torch.float32), (label.view(hw, 3)[None] == colors[:, None]).all(-1).to(torch.float32)

        def matmul():
            return torch.matmul(half[0], half[1].T)

        stages = {
            "pack_mask_bits": (lambda: eng.pack_mask_bits(pred, pp), n * hw + n * words * 8),
            "pack_label_bits": (lambda: eng.pack_label_bits(label, colors, gp), 3 * hw + n * words * 8),
            "mask_pair_counts": (lambda: eng.mask_pair_counts(pp, gp, inter, ad, ag), 2 * (2 * n * words * 8)),
            "coco_match": (lambda: eng.coco_match(inter, ad, ag, scores, order_out=outs[0], match_out=outs[1], dt_ignore_out=outs[2],
                                                  n_valid_out=outs[3], n_kept_out=outs[4]), n * n * 8),
            "chain": (lambda: [stages[k][0]() for k in ("pack_mask_bits", "pack_label_bits", "mask_pair_counts", "coco_match")],
                      n * hw + 3 * hw + 6 * n * words * 8),
            "torch_matmul_f32": (matmul, 2 * n * hw * 4),
            "torch_convert_and_matmul_f32": (lambda: (to_half(), matmul()), n * hw + n * 3 * hw + 2 * 2 * n * hw * 4),
        }
        to_half()
        want = matmul().to(torch.int64)
        ms = {k: [] for k in stages}
        for k, (fn, _) in stages.items():                          # unmeasured first call per arm
            timed(fn)
        assert torch.equal(inter, want), "the pair counts differ from the dense product"
        for _ in range(a.calls):
            for k, (fn, _) in stages.items():
                ms[k].append(timed(fn))
        for k, (_, nbytes) in stages.items():
            med = float(np.median(ms[k]))
            print(json.dumps({"stage": k, "masks": [n, n], "tile": [SIDE, SIDE], "ms_median": round(med, 4), "ms_min": round(min(ms[k]), 4),
                              "bytes_to_move": nbytes, "ms_at_hbm_copy_rate": round(nbytes / (HBM_COPY_TBS * 1e12) * 1e3, 4),
                              "matched_at_0.5": int((outs[1][0, 0] >= 0).sum()) if k in ("coco_match", "chain") else None}), flush=True)
        half[0] = half[1] = None
    eng.close()


def items(n):
    base = [synth.make_image(i) for i in range(8)]
    out = []
    for i in range(n):
        polys, labels = synth.make_rboxes(i, BOXES, SIDE, SIDE)
        cols = np.stack([np.arange(BOXES) + 1, np.full(BOXES, i % 200), np.full(BOXES, 9)], axis=1).astype(np.uint8)
        label = np.zeros((SIDE, SIDE, 3), dtype=np.uint8)
        for p, c in zip(polys, cols):                              # the enclosing box of each rotated box, in its colour
            x0, y0 = np.floor(p.min(0)).astype(int).clip(0, SIDE - 1)
            x1, y1 = np.ceil(p.max(0)).astype(int).clip(0, SIDE - 1)
            label[y0:y1 + 1, x0:x1 + 1] = c
        out.append(driver.WorkItem(f"T{i:05d}", base[i % 8], polys, labels, (label, cols)))
    return out


def run_arm(sam, work, ap):
    pipe = driver.InstancePipeline(sam, 1, prompt="box", multimask=False, gt=True, ap=ap, batch=BATCH, box_batch=BOXES, max_boxes=BOXES,
                                   rle=True)
    matched = [0]

    def sink(res, rel):
        matched[0] += sum(int((r.ap_match[0, 0] >= 0).sum()) for r in res if r.ap_match is not None)
        rel()

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = pipe.run(driver.batched(work, BATCH), sink)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return {"pipeline": "InstancePipeline", "ap": ap, "images": n, "images_per_s": round(n / dt, 1), "seconds": round(dt, 3),
            "matched_at_0.5_per_image": round(matched[0] / max(n, 1), 2)}


def pipeline(a) -> None:
    sd = synth.make_state_dict(synth.CONFIGS[a.model], 0, logit_scale=synth.MARGIN_LOGIT_SCALE)
    sam = samrs_amd.sam_model_registry[a.model](state_dict=sd, precision="f16", max_images=2 * BATCH, max_prompts=64, max_points=1).to("cuda")
    work = items(a.steps * BATCH)
    for arm in (False, True):
        run_arm(sam, work[:3 * BATCH], arm)                        # unmeasured first run per arm
    for rep in range(a.reps):
        for arm in (False, True):
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
        raise SystemExit("coco_ap_bench.py measures on the GPU: no HIP device found")
    if not a.pipeline_only:
        kernels(a)
    if not a.kernels_only:
        pipeline(a)


if __name__ == "__main__":
    main()
