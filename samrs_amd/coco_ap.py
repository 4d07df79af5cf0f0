"""COCO mask AP of instance masks, evaluated on the GPU: the number ``sam_ins_<tag>.json`` / ``gt_ins_<tag>.json`` exist for
(main_sam_rhbox_mask_instance.py:246-255, "Obtain COCO format for AP calculation"), without pycocotools.

    python -m samrs_amd.coco_ap --dt OUT/sam_ins_rhbox.json --gt OUT/gt_ins_rhbox.json --out OUT/ap.json

Per image the device does ``COCOeval.evaluateImg``: the masks become bit planes (``Engine.pack_mask_bits``), every prediction is
counted against every ground truth (``Engine.mask_pair_counts``) and matched greedily for the ten IoU thresholds and four area ranges
at once (``Engine.coco_match``; the rule is stated at samrs_coco_match in include/samrs_hip.h).  ``accumulate`` is then
``COCOeval.accumulate`` + ``summarize`` for one category in numpy float64: the twelve numbers, in COCO's order and wording.

One deliberate difference from pycocotools: a match is a match BY INDEX.  pycocotools stores the matched annotation's ``id`` in
``dtMatches`` and later tests it for truth, so a detection matched to annotation id 0 counts as a false positive;
``gt_ins_<tag>.json`` restarts its ids at 0 per image (instance_to_json.py), so pycocotools would drop the first ship of every image.
Here ground truth 0 is matched like any other, and ``ap.json`` says so (``"matching": "by index"``).  One category, no crowd
annotations (the instance drivers write neither).

Boundary AP (``--boundary``; Cheng et al., CVPR 2021).  Mask IoU is dominated by the interior of a large object: a mask whose outline
is a few pixels off still scores above 0.95 and matches at every threshold.  Boundary AP runs the same matching and accumulation
with the pair score min(mask IoU, boundary IoU), and the rules are (samrs_mask_boundary_bits in include/samrs_hip.h states them):

    python -m samrs_amd.coco_ap --dt OUT/sam_ins_rhbox.json --gt OUT/gt_ins_rhbox.json --boundary --out OUT/boundary_ap.json

* dilation: d = max(1, int(round(ratio * hypot(H, W)))) (``boundary_dilation``), ratio 0.02 by default: 29 for a 1024 x 1024 tile.
* band(M)[y][x] = M[y][x] AND NOT E[y][x], E[y][x] = 1 iff every pixel of the (2 d + 1) x (2 d + 1) square centred on (y, x) lies
  inside the image and is set in M (everything outside the image is background): d iterations of a 3 x 3 all-ones erosion with a
  zero border.
* Boundary IoU(P, G) = |band(P) AND band(G)| / |band(P) OR band(G)|, 0 for an empty union.
* Area ranges, the ground truths' ignore flags and the unmatched detection's ignore flag still use the MASK areas; order, ties,
  min(t, 1 - 1e-10) and the match by index are the mask matching's.
The masks are packed once, banded on the device (``Engine.mask_boundary_bits``), counted twice and matched by the smaller IoU
(``Engine.coco_match(boundary=...)``).  The definition is pinned by the tests to a host statement and to scipy.ndimage, not to cv2.
"""
from __future__ import annotations

import argparse
import json
import math
from typing import Dict, List, Optional, Sequence

import numpy as np

IOU_THRESHOLDS = np.linspace(.5, .95, 10)                       # COCOeval Params.iouThrs
RECALL_THRESHOLDS = np.linspace(.0, 1.0, 101)                   # Params.recThrs
AREA_RANGES = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=np.float64)     # all, small, medium, large
MAX_DETS = (1, 10, 100)
NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR@1", "AR@10", "AR@100", "ARs", "ARm", "ARl")


def image_table(scores, order, match, dt_ignore, n_valid, n_kept: Optional[int] = None) -> dict:
    """One image's matching as ``accumulate`` takes it: scores [nd] (detection order), order [>= n_kept] = detection index per rank,
    match / dt_ignore [A, T, >= n_kept] per rank, n_valid [A].  `n_kept`: the ranks in use (default: the entries of order >= 0)."""
    order = np.asarray(order, dtype=np.int64).reshape(-1)
    k = int((order >= 0).sum()) if n_kept is None else int(n_kept)
    if k < 0:
        raise ValueError("the matching reported a NaN score (n_kept < 0)")
    match, ign = np.asarray(match), np.asarray(dt_ignore)
    return {"scores": np.asarray(scores, dtype=np.float64).reshape(-1), "order": order[:k], "match": match[:, :, :k].astype(np.int64),
            "dt_ignore": ign[:, :, :k].astype(bool), "n_valid": np.asarray(n_valid, dtype=np.int64).reshape(-1)}


def accumulate(per_image_tables: Sequence[dict], max_dets: Sequence[int] = MAX_DETS) -> Dict[str, float]:
    """``COCOeval.accumulate`` + ``summarize`` for one category, numpy float64 -> the twelve numbers by name (``NAMES``).  Per area
    range and maxDet m: each image's first min(m, n_kept) detections, all of them sorted by score (descending, stable); tp = matched
    and not ignored, fp = unmatched and not ignored, cumulative; recall = tp / valid ground truths, precision = tp / (tp + fp + eps)
    made non-increasing from the right and sampled at the first index whose recall reaches each of the 101 recall levels (0 past
    the end).  An area range without valid ground truth stays -1; each number is the mean of its entries > -1, or -1."""
    keys = ("scores", "order", "match", "dt_ignore", "n_valid", "n_kept")
    tabs = [image_table(**{k: t[k] for k in keys if k in t}) for t in per_image_tables]
    A = len(tabs[0]["n_valid"]) if tabs else len(AREA_RANGES)
    T = tabs[0]["match"].shape[1] if tabs else len(IOU_THRESHOLDS)
    R, M = len(RECALL_THRESHOLDS), len(max_dets)
    precision = -np.ones((T, R, A, M))
    recall = -np.ones((T, A, M))
    for a in range(A):
        npig = int(sum(int(t["n_valid"][a]) for t in tabs))
        if npig == 0:
            continue
        for mi, m in enumerate(max_dets):
            sc = np.concatenate([t["scores"][t["order"][:m]] for t in tabs] + [np.zeros(0)])
            dtm = np.concatenate([t["match"][a][:, :m] for t in tabs] + [np.zeros((T, 0), np.int64)], axis=1)
            dig = np.concatenate([t["dt_ignore"][a][:, :m] for t in tabs] + [np.zeros((T, 0), bool)], axis=1)
            inds = np.argsort(-sc, kind="mergesort")
            dtm, dig = dtm[:, inds], dig[:, inds]
            tps = np.logical_and(dtm >= 0, np.logical_not(dig))
            fps = np.logical_and(dtm < 0, np.logical_not(dig))
            tp_sum = np.cumsum(tps, axis=1).astype(np.float64)
            fp_sum = np.cumsum(fps, axis=1).astype(np.float64)
            for t in range(T):
                tp, fp = tp_sum[t], fp_sum[t]
                nd = len(tp)
                rc = tp / npig
                pr = tp / (fp + tp + np.spacing(1))
                recall[t, a, mi] = rc[-1] if nd else 0
                if nd:
                    pr = np.maximum.accumulate(pr[::-1])[::-1]
                at = np.searchsorted(rc, RECALL_THRESHOLDS, side="left")
                q = np.zeros(R)
                ok = at < nd
                q[ok] = pr[at[ok]]
                precision[t, :, a, mi] = q

    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    def thr_index(v):
        hit = np.flatnonzero(np.isclose(IOU_THRESHOLDS[:T], v, rtol=0, atol=1e-9))
        return int(hit[0]) if hit.size and T == len(IOU_THRESHOLDS) else None

    last = M - 1
    out = {"AP": mean(precision[:, :, 0, last])}
    for name, v in (("AP50", .5), ("AP75", .75)):
        k = thr_index(v)
        out[name] = mean(precision[k, :, 0, last]) if k is not None else -1.0
    for name, a in (("APs", 1), ("APm", 2), ("APl", 3)):
        out[name] = mean(precision[:, :, a, last]) if a < A else -1.0
    for mi, m in enumerate(max_dets):
        out[f"AR@{m}"] = mean(recall[:, 0, mi])
    for name, a in (("ARs", 1), ("ARm", 2), ("ARl", 3)):
        out[name] = mean(recall[:, a, last]) if a < A else -1.0
    return out


def summary_lines(numbers: Dict[str, float], max_dets: Sequence[int] = MAX_DETS) -> List[str]:
    """The twelve lines of ``COCOeval.summarize`` in its wording."""
    rows = [("Average Precision", "(AP)", "0.50:0.95", "all", max_dets[-1], "AP"), ("Average Precision", "(AP)", "0.50", "all", max_dets[-1], "AP50"),
            ("Average Precision", "(AP)", "0.75", "all", max_dets[-1], "AP75"), ("Average Precision", "(AP)", "0.50:0.95", "small", max_dets[-1], "APs"),
            ("Average Precision", "(AP)", "0.50:0.95", "medium", max_dets[-1], "APm"), ("Average Precision", "(AP)", "0.50:0.95", "large", max_dets[-1], "APl")]
    rows += [("Average Recall", "(AR)", "0.50:0.95", "all", m, f"AR@{m}") for m in max_dets]
    rows += [("Average Recall", "(AR)", "0.50:0.95", "small", max_dets[-1], "ARs"), ("Average Recall", "(AR)", "0.50:0.95", "medium", max_dets[-1], "ARm"),
             ("Average Recall", "(AR)", "0.50:0.95", "large", max_dets[-1], "ARl")]
    return [" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(t, ty, iou, area, m, numbers[key])
            for t, ty, iou, area, m, key in rows]


BOUNDARY_IOU = "min(mask, boundary)"
DILATION_RATIO = 0.02


def boundary_dilation(h: int, w: int, ratio: float = DILATION_RATIO) -> int:
    """The band's width d for H x W masks: max(1, int(round(ratio * hypot(H, W)))) -- 29 for 1024 x 1024 and for 800 x 1200."""
    return max(1, int(round(float(ratio) * math.hypot(int(h), int(w)))))


def boundary_miou(band_inter, band_area_d, band_area_g) -> Dict[str, float]:
    """Boundary mIoU over objects from their diagonal band counts: "average" = the mean of inter / union per object (0 for an empty
    union), "area" = sum of inter / sum of union."""
    i = np.asarray(band_inter, dtype=np.int64).reshape(-1)
    u = np.asarray(band_area_d, dtype=np.int64).reshape(-1) + np.asarray(band_area_g, dtype=np.int64).reshape(-1) - i
    per = np.divide(i.astype(np.float64), u.astype(np.float64), out=np.zeros(len(i)), where=u > 0)
    return {"average": float(per.mean()) if len(per) else 0.0, "area": float(i.sum() / u.sum()) if u.sum() > 0 else 0.0}


def boundary_heading(dilation_ratio: float = DILATION_RATIO) -> str:
    """The line printed above the twelve lines of a Boundary AP."""
    return f"Boundary AP (IoU = {BOUNDARY_IOU}, dilation ratio {float(dilation_ratio):g}):"


def ap_record(numbers: Dict[str, float], tables: Sequence[dict], boundary: bool = False, dilation_ratio: float = DILATION_RATIO,
              miou: Optional[Dict[str, float]] = None) -> dict:
    """What ``ap.json`` holds: the twelve numbers, the counts and how matches are told.  `boundary`: a Boundary AP record
    (``boundary_ap.json``) also says which IoU was matched on, the dilation ratio and, where known (`miou`, ``boundary_miou``'s
    result), the Boundary mIoU.  A mask record is what it always was."""
    rec = {k: float(numbers[k]) for k in numbers}
    rec.update(n_images=len(tables), n_gt=int(sum(int(np.asarray(t["n_valid"]).reshape(-1)[0]) for t in tables)),
               n_dt=int(sum(len(np.asarray(t["scores"]).reshape(-1)) for t in tables)), matching="by index")
    if boundary:
        rec.update(iou=BOUNDARY_IOU, dilation_ratio=float(dilation_ratio))
        if miou is not None:
            rec["boundary_miou"] = {k: float(miou[k]) for k in ("average", "area")}
    return rec


def match_image(engine, pred_masks, scores, gt_masks, max_det: int = MAX_DETS[-1], boundary: bool = False,
                dilation_ratio: float = DILATION_RATIO) -> dict:
    """One image on the device -> its table (``image_table``).  pred_masks [nd, H, W] and gt_masks [ng, H, W]: bool / uint8 arrays
    or tensors (uploaded when they are on the host); scores [nd].  `boundary`: the Boundary AP table instead -- the planes are
    banded with d = ``boundary_dilation(H, W, dilation_ratio)``, counted a second time and matched by min(mask IoU, boundary IoU)."""
    import torch

    def dev(m):
        if not isinstance(m, torch.Tensor):
            m = torch.from_numpy(np.ascontiguousarray(np.asarray(m) != 0).view(np.uint8))
        return m.to(engine.device).contiguous()
    p, g = dev(pred_masks), dev(gt_masks)
    if p.shape[0] and g.shape[0] and p.shape[1:] != g.shape[1:]:
        raise ValueError(f"predictions {tuple(p.shape[1:])} and ground truth {tuple(g.shape[1:])} differ in size")
    hw = p.shape[1:] if p.shape[0] else g.shape[1:]
    words = (int(hw[0]) * int(hw[1]) + 63) // 64 if len(hw) == 2 and hw[0] * hw[1] else 1
    empty = lambda: torch.zeros(0, words, dtype=torch.int64, device=engine.device)
    pa = engine.pack_mask_bits(p) if p.shape[0] else empty()
    ga = engine.pack_mask_bits(g) if g.shape[0] else empty()
    inter, ad, ag = engine.mask_pair_counts(pa, ga)
    sc = np.asarray(scores.cpu() if isinstance(scores, torch.Tensor) else scores, dtype=np.float32).reshape(-1)
    band = None
    if boundary:
        if len(hw) == 2 and hw[0] * hw[1]:
            d = boundary_dilation(hw[0], hw[1], dilation_ratio)
            pa, ga = engine.mask_boundary_bits(pa, hw[0], hw[1], d), engine.mask_boundary_bits(ga, hw[0], hw[1], d)
        band = engine.mask_pair_counts(pa, ga)
    order, match, ign, n_valid, n_kept = engine.coco_match(inter, ad, ag, sc, max_det=max_det, boundary=band)
    return image_table(sc, order.cpu().numpy(), match.cpu().numpy(), ign.cpu().numpy(), n_valid.cpu().numpy(), int(n_kept.cpu()[0]))


def evaluate_masks(engine, images, max_dets: Sequence[int] = MAX_DETS, boundary: bool = False, dilation_ratio: float = DILATION_RATIO):
    """`images`: (pred_masks, scores, gt_masks) per image -> (the twelve numbers, the per-image tables); `boundary`: Boundary AP."""
    tables = [match_image(engine, p, s, g, max_det=max(max_dets), boundary=boundary, dilation_ratio=dilation_ratio) for p, s, g in images]
    return accumulate(tables, max_dets), tables


def load_coco_files(dt_path: str, gt_path: str):
    """(image ids in the ground-truth file's order, id -> list of (score, rle), id -> list of rle) of a results file and a dataset
    file as ``samrs_amd.instances`` writes them."""
    with open(dt_path) as f:
        dt = json.load(f)
    with open(gt_path) as f:
        gt = json.load(f)
    ids = [im["id"] for im in gt["images"]]
    dts = {i: [] for i in ids}
    gts = {i: [] for i in ids}
    for d in dt:
        dts.setdefault(d["image_id"], []).append((float(d["score"]), d["segmentation"]))
    for g in gt["annotations"]:
        gts.setdefault(g["image_id"], []).append(g["segmentation"])
    return [i for i in dts if i in gts], dts, gts


def evaluate_files(engine, dt_path: str, gt_path: str, boundary: bool = False, dilation_ratio: float = DILATION_RATIO):
    """Any pair of such files on the GPU: per image the RLE strings are uploaded as they are and decoded on the device
    (``samrs_amd.rle.decode_device``, samrs_rle_decode); the masks never exist on the host.  `boundary`: Boundary AP."""
    import torch
    from . import rle
    ids, dts, gts = load_coco_files(dt_path, gt_path)

    def images():
        for i in ids:
            size = (dts[i][0][1] if dts[i] else gts[i][0])["size"] if (dts[i] or gts[i]) else [1, 1]
            stack = lambda segs: (rle.decode_device(engine, segs) if segs
                                  else torch.zeros(0, size[0], size[1], dtype=torch.uint8, device=engine.device))
            yield stack([s for _, s in dts[i]]), np.array([sc for sc, _ in dts[i]], dtype=np.float32), stack(gts[i])
    return evaluate_masks(engine, images(), boundary=boundary, dilation_ratio=dilation_ratio)


def main(argv=None):
    ap = argparse.ArgumentParser(description="COCO mask AP of sam_ins_<tag>.json against gt_ins_<tag>.json, evaluated on the GPU")
    ap.add_argument("--dt", required=True, help="COCO results file (sam_ins_<tag>.json)")
    ap.add_argument("--gt", required=True, help="COCO dataset file (gt_ins_<tag>.json)")
    ap.add_argument("--out", default=None, help="write the record here (ap.json; with --boundary: boundary_ap.json)")
    ap.add_argument("--model", default="vit_tiny", help="the engine that hosts the kernels (no weights are used)")
    ap.add_argument("--boundary", action="store_true",
                    help="Boundary AP: match on min(mask IoU, boundary IoU), the bands computed on the GPU (samrs_mask_boundary_bits)")
    ap.add_argument("--dilation-ratio", type=float, default=DILATION_RATIO, metavar="R",
                    help="with --boundary: the band's width as a fraction of the image diagonal (default 0.02)")
    args = ap.parse_args(argv)
    if not (args.dilation_ratio > 0):
        ap.error("--dilation-ratio must be > 0")
    import samrs_amd
    sam = samrs_amd.sam_model_registry[args.model](max_prompts=1).to("cuda:0")
    numbers, tables = evaluate_files(sam.engine, args.dt, args.gt, boundary=args.boundary, dilation_ratio=args.dilation_ratio)
    if args.boundary:
        print(boundary_heading(args.dilation_ratio), flush=True)
    for line in summary_lines(numbers):
        print(line, flush=True)
    rec = ap_record(numbers, tables, boundary=args.boundary, dilation_ratio=args.dilation_ratio)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f)
    return rec


if __name__ == "__main__":
    main()
