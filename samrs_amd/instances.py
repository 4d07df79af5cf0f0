"""Drop-in for the reference's HRSC2016 instance drivers (``Generate Dataset/main_sam_hbox_mask_instance.py``,
``main_sam_rbox_mask_instance.py``, ``main_sam_rhbox_mask_instance.py``): images + HRSC XML annotations (+ the ground-truth
label images) in; ``sam_ins_<tag>.json`` (the predictions as COCO results), ``gt_ins_<tag>.json`` (the ground truth as a COCO
dataset, ``instance_to_json.py:5-108``), ``miou.json`` and the printed ``Average mIOU: ... Area mIOU: ...`` line
(main_sam_rhbox_mask_instance.py:202-255) out.

    torchrun --nproc-per-node 8 -m samrs_amd.instances --images DIR --annotations DIR --gt-labels DIR --out OUT \\
             --prompt box --model vit_h --checkpoint sam_vit_h_4b8939.pth

``--prompt point`` is main_sam_hbox_mask_instance.py (tag ``hbox``), ``rbox_mask`` main_sam_rbox_mask_instance.py (tag ``rbox``),
``box`` main_sam_rhbox_mask_instance.py (tag ``rhbox``); all three use ``multimask_output=False`` like the reference,
``--multimask`` keeps the best of the three multimask outputs instead (BASELINE.json configs[3]).

The GPU side is ``driver.InstancePipeline(gt=True, rle=True)``: the masks stay in HBM; per instance the host receives its
quality, its area, |mask AND ground truth|, |ground truth| and the two COCO RLE strings, all computed on the device
(``samrs_select_best``, ``samrs_gt_match``, ``samrs_rle_encode``).  Each rank writes one fragment per image
(``OUT/parts/<stem>.json``); after a barrier rank 0 merges them in sorted-stem order.

``--ap`` (needs ``--gt-labels``) adds the number the two JSON files exist for (main_sam_rhbox_mask_instance.py:246-255): on the
device every prediction of an image is matched against every ground truth of it (``InstancePipeline(ap=True)``), each fragment
gains an ``"ap"`` record, rank 0 writes ``ap.json`` and prints COCO's twelve lines after the mIoU line (``samrs_amd.coco_ap``; a
match is a match by index, so ground truth 0 counts).

``--boundary`` (needs ``--ap``) adds Boundary AP and Boundary mIoU (Cheng et al., CVPR 2021; the rules: samrs_mask_boundary_bits in
include/samrs_hip.h): mask IoU is dominated by an object's interior, these respond to its outline.  The bands are computed on the
device (``InstancePipeline(boundary=True)``), each fragment gains ``"boundary_ap"`` and the per-object band counts, rank 0 writes
``boundary_ap.json`` and prints the twelve lines and one ``Boundary mIOU`` line after the existing output.  ``miou.json``,
``ap.json`` and the two COCO files are unchanged.

One deliberate difference from the reference: image ids follow the SORTED image stems.  The reference numbers images in
``os.listdir`` order (main_sam_rhbox_mask_instance.py:83), which is unspecified.  Images without an annotation file are ignored.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import xml.etree.ElementTree as ET
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

TAGS = {"point": "hbox", "rbox_mask": "rbox", "box": "rhbox"}
IMAGE_EXTS = (".png", ".jpg", ".jpeg", ".tif", ".bmp")


# ------------------------------------------------------------------------------------------------
# HRSC XML (loaddata.load_hrsc, loaddata.py:41-102)
# ------------------------------------------------------------------------------------------------
@dataclass
class HrscImage:
    """The objects of one HRSC image.  ``skip``: the reference's ``error == 1`` (an object whose seg_color does not have three
    fields, or no objects at all); such an image appears in no output (main_sam_rhbox_mask_instance.py:114-117)."""
    hboxes: np.ndarray      # float32 [n, 4] box_xmin, box_ymin, box_xmax, box_ymax
    rboxes: np.ndarray      # float32 [n, 4, 2] le90 corners, best begin point first
    colors: np.ndarray      # uint8 [n, 3] seg_color
    points: np.ndarray      # float32 [n, 2] mbox_cx, mbox_cy
    skip: bool


def _line_length(p, q) -> float:
    return math.sqrt(math.pow(p[0] - q[0], 2) + math.pow(p[1] - q[1], 2))


def _best_begin_point(poly: Sequence[float]) -> List[float]:
    """Rotate the four corners so that the sum of distances to (xmin, ymin), (xmax, ymin), (xmax, ymax), (xmin, ymax) is
    smallest, the first minimum winning (mmrotate's get_best_begin_point_single); double precision on the float32 corners."""
    pts = [(poly[2 * k], poly[2 * k + 1]) for k in range(4)]
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    dst = [(min(xs), min(ys)), (max(xs), min(ys)), (max(xs), max(ys)), (min(xs), max(ys))]
    force, flag = 100000000.0, 0
    for i in range(4):
        rot = pts[i:] + pts[:i]
        f = _line_length(rot[0], dst[0]) + _line_length(rot[1], dst[1]) + _line_length(rot[2], dst[2]) + _line_length(rot[3], dst[3])
        if f < force:
            force, flag = f, i
    rot = pts[flag:] + pts[:flag]
    return [c for p in rot for c in p]


def le90_corners(cx: float, cy: float, w: float, h: float, ang: float) -> np.ndarray:
    """(cx, cy, w, h, angle) -> float32 [4, 2] corners by the le90 formula (utils/transform.py:193-216) in float32, in the
    reference's order of operations and array shapes (one [1, 1] array per value), then the best begin point (:234-280)."""
    rb = np.array([[cx, cy, w, h, ang, 0]], dtype=np.float32)
    center, bw, bh, theta = rb[:, 0:2], rb[:, 2:3], rb[:, 3:4], rb[:, 4:5]
    cos, sin = np.cos(theta), np.sin(theta)
    v1 = np.concatenate([bw / 2 * cos, bw / 2 * sin], axis=-1)
    v2 = np.concatenate([-bh / 2 * sin, bh / 2 * cos], axis=-1)
    poly = np.concatenate([center - v1 - v2, center + v1 - v2, center + v1 + v2, center - v1 + v2], axis=-1)
    return np.asarray(_best_begin_point(poly[0].tolist()), dtype=np.float32).reshape(4, 2)


def read_hrsc_xml(path: str) -> HrscImage:
    """One HRSC2016 annotation file (``HRSC_Objects/HRSC_Object``)."""
    root = ET.parse(path).getroot()
    hb, rb, col, pt = [], [], [], []
    skip = False
    for obj in root.findall("HRSC_Objects/HRSC_Object"):
        f = lambda tag: float(obj.find(tag).text)
        hb.append(np.array([f("box_xmin"), f("box_ymin"), f("box_xmax"), f("box_ymax")], dtype=np.float32))
        rb.append(le90_corners(f("mbox_cx"), f("mbox_cy"), f("mbox_w"), f("mbox_h"), f("mbox_ang")))
        text = obj.find("seg_color").text
        fields = text.split(",") if text is not None else []
        if len(fields) != 3:
            skip = True
            col.append(np.zeros(3, dtype=np.uint8))
        else:
            col.append(np.array([int(v) for v in fields], dtype=np.uint8))
        pt.append(np.array([f("mbox_cx"), f("mbox_cy")], dtype=np.float32))
    if not rb:
        skip = True
    n = len(rb)
    return HrscImage(np.stack(hb) if n else np.zeros((0, 4), np.float32), np.stack(rb) if n else np.zeros((0, 4, 2), np.float32),
                     np.stack(col) if n else np.zeros((0, 3), np.uint8), np.stack(pt) if n else np.zeros((0, 2), np.float32), skip)


def list_images(images_dir: str, annotations_dir: str) -> Tuple[List[str], Dict[str, str], Dict[str, HrscImage]]:
    """(sorted stems of the images that are evaluated, stem -> image file name, stem -> annotations).  Images without
    ``<stem>.xml`` are ignored; images the reference skips (HrscImage.skip) are left out."""
    files = {os.path.splitext(f)[0]: f for f in os.listdir(images_dir) if f.lower().endswith(IMAGE_EXTS)}
    stems, anns = [], {}
    for stem in sorted(files):
        path = os.path.join(annotations_dir, stem + ".xml")
        if not os.path.exists(path):
            continue
        a = read_hrsc_xml(path)
        if a.skip:
            continue
        stems.append(stem)
        anns[stem] = a
    return stems, files, anns


# ------------------------------------------------------------------------------------------------
# Fragments, mIoU and the COCO files
# ------------------------------------------------------------------------------------------------
def fragment_path(out_dir: str, stem: str) -> str:
    return os.path.join(out_dir, "parts", stem + ".json")


def write_fragment(out_dir: str, stem: str, frag: dict) -> None:
    """One image's results; written through a rename, so that --resume can take its presence as "this image is complete"."""
    os.makedirs(os.path.join(out_dir, "parts"), exist_ok=True)
    tmp = fragment_path(out_dir, stem) + f".tmp.{os.getpid()}"
    with open(tmp, "w") as f:
        json.dump(frag, f)
    os.replace(tmp, fragment_path(out_dir, stem))


def make_fragment(height: int, width: int, scores, rles: Sequence[str], pred_area=None, inter=None, gt_area=None,
                  gt_rles: Optional[Sequence[str]] = None, bboxes=None, gt_bboxes=None, ap: Optional[dict] = None,
                  boundary: Optional[dict] = None) -> dict:
    """scores: fp32 qualities (stored as float(fp32), instance_to_json.py:103); rles / gt_rles: the COCO counts strings; bboxes /
    gt_bboxes (--mask-boxes): COCO [x, y, w, h] per prediction / ground-truth mask; ap (--ap): the image's matching tables
    (``TileResult.ap_tables``), stored as the ranks in use: order, match, dt_ignore, n_valid; boundary (--boundary): the same of the
    Boundary AP matching (``TileResult.boundary_tables``) as "boundary_ap", and its three per-object band counts."""
    frag = {"height": int(height), "width": int(width), "scores": [float(np.float32(s)) for s in scores], "rles": list(rles)}
    if gt_rles is not None:
        frag.update(pred_area=[int(v) for v in pred_area], inter=[int(v) for v in inter], gt_area=[int(v) for v in gt_area],
                    gt_rles=list(gt_rles))
    if bboxes is not None:
        frag["bboxes"] = [[int(v) for v in b] for b in bboxes]
    if gt_bboxes is not None:
        frag["gt_bboxes"] = [[int(v) for v in b] for b in gt_bboxes]
    if ap is not None:
        k = int(ap["n_kept"])
        if k < 0:
            raise ValueError("a predicted IoU is NaN: the matching cannot order the detections")
        frag["ap"] = {"order": np.asarray(ap["order"])[:k].tolist(), "match": np.asarray(ap["match"])[:, :, :k].tolist(),
                      "dt_ignore": np.asarray(ap["dt_ignore"])[:, :, :k].tolist(), "n_valid": np.asarray(ap["n_valid"]).tolist()}
    if boundary is not None:
        k = int(boundary["n_kept"])
        if k < 0:
            raise ValueError("a predicted IoU is NaN: the matching cannot order the detections")
        frag["boundary_ap"] = {"order": np.asarray(boundary["order"])[:k].tolist(), "match": np.asarray(boundary["match"])[:, :, :k].tolist(),
                               "dt_ignore": np.asarray(boundary["dt_ignore"])[:, :, :k].tolist(),
                               "n_valid": np.asarray(boundary["n_valid"]).tolist()}
        for key in ("band_inter", "band_area_d", "band_area_g"):
            frag[key] = [int(v) for v in boundary[key]]
    return frag


def coco_bboxes(hbox: np.ndarray, areas) -> List[List[int]]:
    """int32 [n, 4] inclusive xmin, ymin, xmax, ymax -> COCO [x, y, w, h] in whole pixels; [0, 0, 0, 0] for an empty mask."""
    return [[int(b[0]), int(b[1]), int(b[2] - b[0] + 1), int(b[3] - b[1] + 1)] if int(a) > 0 else [0, 0, 0, 0]
            for b, a in zip(hbox, areas)]


def pending_stems(out_dir: str, stems: Sequence[str], need_ap: bool = False, need_boundary: bool = False) -> List[str]:
    """--resume: the stems whose fragment is not on disk yet; with `need_ap` (--ap) a fragment without an "ap" record (written by
    a run without the flag) counts as not done, and with `need_boundary` (--boundary) one without a "boundary_ap" record."""
    def done(s):
        path = fragment_path(out_dir, s)
        if not os.path.exists(path):
            return False
        if not (need_ap or need_boundary):
            return True
        with open(path) as f:
            frag = json.load(f)
        return (not need_ap or "ap" in frag) and (not need_boundary or "boundary_ap" in frag)
    return [s for s in stems if not done(s)]


def miou_from_tallies(inter: Sequence[int], pred_area: Sequence[int], gt_area: Sequence[int]) -> Tuple[float, float, int]:
    """``driver.mean_iou`` from per-instance integers (main_sam_rhbox_mask_instance.py:221-242): union = pred + gt - inter;
    instances with an empty union are left out.  Returns (Average mIOU, Area mIOU, instances averaged)."""
    ious, inter_all, union_all = [], [], []
    for i, p, g in zip(inter, pred_area, gt_area):
        union = float(int(p) + int(g) - int(i))
        if union > 0:
            inter_all.append(float(i))
            union_all.append(union)
            ious.append(float(i) / union)
    if not ious:
        return float("nan"), float("nan"), 0
    return float(np.mean(ious)), float(np.sum(inter_all) / np.sum(union_all)), len(ious)


def fragment_tables(out_dir: str, stems: Sequence[str], frags: Sequence[dict], key: str, flag: str) -> List[dict]:
    """The fragments' matching tables under `key` ("ap" / "boundary_ap") as ``coco_ap.accumulate`` takes them."""
    from . import coco_ap
    tables = []
    for stem, fr in zip(stems, frags):
        if key not in fr:
            raise RuntimeError(f"fragment {fragment_path(out_dir, stem)} holds no \"{key}\" record: written without {flag} (rerun with --resume)")
        t = fr[key]
        k, A, T = len(t["order"]), len(t["n_valid"]), len(coco_ap.IOU_THRESHOLDS)
        tables.append(coco_ap.image_table(fr["scores"], t["order"], np.asarray(t["match"], dtype=np.int64).reshape(A, T, k),
                                          np.asarray(t["dt_ignore"], dtype=np.uint8).reshape(A, T, k), t["n_valid"], k))
    return tables


def merge_fragments(out_dir: str, stems: Sequence[str], tag: str, with_gt: bool, with_ap: bool = False, with_boundary: bool = False,
                    dilation_ratio: float = 0.02) -> Optional[dict]:
    """Rank 0, after every rank has written its fragments: ``sam_ins_<tag>.json`` (binary_to_coco_pre_hrsc) and, with the
    ground truth, ``gt_ins_<tag>.json`` (binary_to_coco_gt_hrsc) and ``miou.json``; image id = position in `stems` (sorted),
    annotation ids restart at 0 per image.  `with_ap`: also ``ap.json`` from the fragments' matching tables
    (``coco_ap.accumulate``) and COCO's twelve lines after the mIoU line.  `with_boundary`: also ``boundary_ap.json`` from the
    "boundary_ap" tables and the band counts -- the twelve Boundary AP numbers and the Boundary mIoU over the objects ``miou.json``
    covers (those with a non-empty mask union) -- printed after everything else.  Returns the mIoU record (None without ground truth)."""
    frags = []
    for stem in stems:
        path = fragment_path(out_dir, stem)
        if not os.path.exists(path):
            raise RuntimeError(f"missing fragment {path}: a rank did not finish (rerun with --resume)")
        with open(path) as f:
            frags.append(json.load(f))
    pred = []
    for n, fr in enumerate(frags):
        size = [fr["height"], fr["width"]]
        for c, (counts, score) in enumerate(zip(fr["rles"], fr["scores"])):
            pred.append({"image_id": int(n), "category_id": 0, "segmentation": {"size": size, "counts": counts}, "score": float(score)})
            if "bboxes" in fr:                                     # --mask-boxes (the reference left it out: instance_to_json.py:63)
                pred[-1]["bbox"] = fr["bboxes"][c]
    with open(os.path.join(out_dir, f"sam_ins_{tag}.json"), "w") as f:
        json.dump(pred, f)
    if not with_gt:
        return None
    gt = {"images": [], "annotations": [], "categories": [{"id": 0, "name": "ship", "supercategory": "None"}]}
    for n, (stem, fr) in enumerate(zip(stems, frags)):
        gt["images"].append({"id": int(n), "width": int(fr["width"]), "height": int(fr["height"]), "file_name": "{}.png".format(stem)})
    inter, parea, garea = [], [], []
    for n, fr in enumerate(frags):
        size = [fr["height"], fr["width"]]
        for c, counts in enumerate(fr["gt_rles"]):
            gt["annotations"].append({"id": c, "image_id": n, "category_id": 0, "area": int(fr["gt_area"][c]), "iscrowd": 0,
                                      "segmentation": {"size": size, "counts": counts}, "attributes": {}})
            if "gt_bboxes" in fr:
                gt["annotations"][-1]["bbox"] = fr["gt_bboxes"][c]
        inter += fr["inter"]
        parea += fr["pred_area"]
        garea += fr["gt_area"]
    with open(os.path.join(out_dir, f"gt_ins_{tag}.json"), "w") as f:
        json.dump(gt, f)
    avg, area, k = miou_from_tallies(inter, parea, garea)
    rec = {"average": None if math.isnan(avg) else avg, "area": None if math.isnan(area) else area, "n_instances": k}
    with open(os.path.join(out_dir, "miou.json"), "w") as f:
        json.dump(rec, f)
    print("Average mIOU: ", avg, "Area mIOU: ", area, flush=True)              # main_sam_rhbox_mask_instance.py:244
    if with_ap:
        from . import coco_ap
        tables = fragment_tables(out_dir, stems, frags, "ap", "--ap")
        numbers = coco_ap.accumulate(tables)
        with open(os.path.join(out_dir, "ap.json"), "w") as f:
            json.dump(coco_ap.ap_record(numbers, tables), f)
        for line in coco_ap.summary_lines(numbers):
            print(line, flush=True)
    if with_boundary:
        from . import coco_ap
        tables = fragment_tables(out_dir, stems, frags, "boundary_ap", "--boundary")
        numbers = coco_ap.accumulate(tables)
        bi, bd, bg = ([v for fr in frags for v in fr[key]] for key in ("band_inter", "band_area_d", "band_area_g"))
        covered = [j for j, (i, p, g) in enumerate(zip(inter, parea, garea)) if int(p) + int(g) - int(i) > 0]       # miou.json's objects
        bm = coco_ap.boundary_miou([bi[j] for j in covered], [bd[j] for j in covered], [bg[j] for j in covered])
        with open(os.path.join(out_dir, "boundary_ap.json"), "w") as f:
            json.dump(coco_ap.ap_record(numbers, tables, boundary=True, dilation_ratio=dilation_ratio, miou=bm), f)
        print(coco_ap.boundary_heading(dilation_ratio), flush=True)
        for line in coco_ap.summary_lines(numbers):
            print(line, flush=True)
        print("Boundary mIOU: Average ", bm["average"], "Area ", bm["area"], flush=True)
    return rec


# ------------------------------------------------------------------------------------------------
# The run
# ------------------------------------------------------------------------------------------------
def run(args) -> Optional[dict]:
    """The whole CLI; returns rank 0's mIoU record (None on other ranks and without --gt-labels)."""
    import torch
    import torch.distributed as dist
    import samrs_amd
    from . import driver, generate, tile_io

    if args.prompt not in TAGS:
        raise ValueError(f"--prompt must be one of {sorted(TAGS)}")
    tag = TAGS[args.prompt]
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    share = os.environ.get("SAMRS_SHARE_GPU") == "1"          # every rank on cuda:0, collectives over gloo (generate.run)
    if share:
        local = 0
    torch.cuda.set_device(local)
    if world > 1 and not dist.is_initialized():
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    with_gt = bool(getattr(args, "gt_labels", None))
    with_ap = bool(getattr(args, "ap", False))
    if with_ap and not with_gt:
        raise ValueError("--ap matches the predictions against the ground truth: it needs --gt-labels")
    with_boundary = bool(getattr(args, "boundary", False))
    ratio = float(getattr(args, "dilation_ratio", 0.02))
    if with_boundary and not with_ap:
        raise ValueError("--boundary is a second matching beside the mask AP's: it needs --ap")
    stems, files, anns = list_images(args.images, args.annotations)
    todo = stems
    if getattr(args, "resume", False):
        # listed once, on rank 0, and broadcast (generate.run: ranks must index the same list)
        todo = driver.agree_on_list(pending_stems(args.out, stems, need_ap=with_ap, need_boundary=with_boundary) if rank == 0 else [])
        if rank == 0:
            print(f"[rank 0] --resume: {len(stems) - len(todo)} of {len(stems)} images already complete", flush=True)
    batch = getattr(args, "batch", 8)
    multimask = bool(getattr(args, "multimask", False))
    split = getattr(args, "split", None)
    # single-mask: the 1x-rate operand split unless --split / SAMRS_SPLIT say otherwise (generate.default_split_options); multimask:
    # the model's own multimask-grade default
    opts = generate.default_split_options(split) if not multimask else ({"split": int(split)} if split is not None else None)
    sam = samrs_amd.sam_model_registry[args.model](checkpoint=args.checkpoint, precision=getattr(args, "precision", "f16"), options=opts,
                                                   audit_passes=getattr(args, "audit_passes", 0),
                                                   max_images=2 * batch, max_prompts=args.box_batch).to(f"cuda:{local}")
    max_boxes = max([len(anns[s].colors) for s in stems] + [1])
    pipe = driver.InstancePipeline(sam, 1, prompt=args.prompt, multimask=multimask, fill_rule=getattr(args, "fill_rule", "auto"),
                                   gt=with_gt, batch=batch, box_batch=args.box_batch, max_boxes=max_boxes, rle=True,
                                   rle_buffer_mb=getattr(args, "rle_buffer_mb", 256), keep_masks=False,
                                   batch_decode=True if getattr(args, "batch_decode", False) else "auto",
                                   min_region_area=int(getattr(args, "min_region_area", 0) or 0),
                                   region_mode=getattr(args, "region_mode", "both"),
                                   mask_boxes=bool(getattr(args, "mask_boxes", False)), ap=with_ap,
                                   **(dict(boundary=True, dilation_ratio=ratio) if with_boundary else {}))
    os.makedirs(os.path.join(args.out, "parts"), exist_ok=True)
    import zlib
    wq_name = "samrs_ins/%08x" % zlib.crc32(("\n".join(todo) + "|" + args.out).encode())
    wq = driver.WorkQueue(len(todo), chunk=batch, rank=rank, world=world, mode=getattr(args, "schedule", "static"), name=wq_name)

    def load(stem: str) -> driver.WorkItem:
        a = anns[stem]
        img = tile_io.read_rgb(os.path.join(args.images, files[stem]))
        ann = a.points if args.prompt == "point" else a.rboxes
        gt = None
        if with_gt:
            gt = (tile_io.read_rgb(os.path.join(args.gt_labels, stem + ".png")), a.colors)
        return driver.WorkItem(stem, img, ann, np.zeros(len(a.colors), dtype=np.int64), gt)

    def batches():
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=2) as readers:    # decode of the next batch overlaps the GPU work on this one
            nxt = None
            for s0, s1 in wq:
                fut = [readers.submit(load, st) for st in todo[s0:s1]]
                if nxt is not None:
                    yield [f.result() for f in nxt]
                nxt = fut
            if nxt is not None:
                yield [f.result() for f in nxt]

    def sink(results, release):
        try:
            for r in results:
                n = len(r.labels)
                rles = [r.rle(j)["counts"] for j in range(n)]
                bbs = coco_bboxes(r.mask_hbox, r.areas) if r.mask_hbox is not None else None
                if with_gt:
                    gbs = coco_bboxes(r.gt_hbox, r.gt_area) if r.gt_hbox is not None else None
                    frag = make_fragment(r.size[0], r.size[1], r.quality, rles, r.areas, r.inter, r.gt_area,
                                         [r.gt_rle(j)["counts"] for j in range(n)], bbs, gbs, ap=r.ap_tables,
                                         boundary=r.boundary_tables)
                else:
                    frag = make_fragment(r.size[0], r.size[1], r.quality, rles, bboxes=bbs)
                write_fragment(args.out, r.key, frag)
        finally:
            release()

    import time
    t0 = time.perf_counter()
    n_done = pipe.run(batches(), sink)
    wall = time.perf_counter() - t0
    print(f"[rank {rank}] {n_done} images in {wall:.2f} s = {n_done / max(wall, 1e-9):.1f} images/s", flush=True)
    if world > 1:
        dist.barrier()
    rec = None
    if rank == 0:
        rec = merge_fragments(args.out, stems, tag, with_gt, with_ap, with_boundary, ratio)
        if getattr(args, "audit_passes", 0) > 0 and sam.finish_audit() is not None:
            from . import audit
            audit.write_json(sam.audit_report, os.path.join(args.out, "statistic", "audit.json"))
    if world > 1:
        dist.barrier()                                         # nobody leaves before the merged files are on disk
    return rec


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="SAM instance masks + ground-truth evaluation on HRSC2016 (SAMRS) on MI355X")
    ap.add_argument("--images", required=True, help="image directory (HRSC: .bmp)")
    ap.add_argument("--annotations", required=True, help="HRSC XML directory (<stem>.xml)")
    ap.add_argument("--gt-labels", default=None, help="ground-truth label images <stem>.png (instance j = pixels of its seg_color); "
                    "without it only sam_ins_<tag>.json is written")
    ap.add_argument("--out", required=True)
    ap.add_argument("--prompt", required=True, choices=sorted(TAGS), help="point = main_sam_hbox_mask_instance.py (tag hbox), "
                    "rbox_mask = main_sam_rbox_mask_instance.py (tag rbox), box = main_sam_rhbox_mask_instance.py (tag rhbox)")
    ap.add_argument("--multimask", action="store_true", help="keep the best of the three multimask outputs (BASELINE.json configs[3]); "
                    "the reference uses multimask_output=False")
    ap.add_argument("--model", default="vit_h")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--precision", default="f16", choices=["f16", "bf16"])
    ap.add_argument("--split", type=int, default=None, help="engine operand-split mode (DESIGN.md section 2)")
    ap.add_argument("--audit-passes", type=int, default=0, metavar="N",
                    help="profile the operand ranges of the first N encoder passes (samrs_amd.audit): a warning names tensors that saturate "
                         "the operand type, rank 0 writes OUT/statistic/audit.json; recommended (4) for a new checkpoint, 0 = off")
    ap.add_argument("--fill-rule", default="auto", help="rbox_mask: cv2.fillPoly span rule (transforms.resolve_fill_rule)")
    ap.add_argument("--batch", type=int, default=8, help="tiles per encoder pass")
    ap.add_argument("--box-batch", type=int, default=64, help="objects per predict call")
    ap.add_argument("--rle-buffer-mb", type=int, default=256)
    ap.add_argument("--schedule", default="static", choices=["static", "dynamic"])
    ap.add_argument("--resume", action="store_true", help="skip images whose fragment OUT/parts/<stem>.json already exists")
    ap.add_argument("--ap", action="store_true",
                    help="COCO mask AP on the GPU (needs --gt-labels): every prediction of an image is matched against every ground "
                         "truth of it on the device; OUT/ap.json holds the twelve COCO numbers, printed after the mIoU line "
                         "(samrs_amd.coco_ap; a match is a match by index)")
    ap.add_argument("--boundary", action="store_true",
                    help="Boundary AP and Boundary mIoU on the GPU (needs --ap): the matching on min(mask IoU, boundary IoU) beside the "
                         "mask AP's; OUT/boundary_ap.json holds the twelve numbers and the Boundary mIoU, printed after the existing output")
    ap.add_argument("--dilation-ratio", type=float, default=0.02, metavar="R",
                    help="with --boundary: the band's width as a fraction of the image diagonal (default 0.02)")
    ap.add_argument("--batch-decode", action="store_true",
                    help="decode the prompts of all images of a batch in one decoder chain (Engine.predict_multi); same outputs")
    from . import generate
    generate.add_region_arguments(ap)
    generate.add_mask_box_arguments(ap, "every prediction of sam_ins_<tag>.json gains \"bbox\" (COCO [x, y, w, h]), and so does every "
                                        "ground-truth annotation with --gt-labels")
    return ap


def parse_args(argv=None):
    """The arguments, with the usage errors that need no device: --boundary without --ap, a dilation ratio that is not positive."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.boundary and not args.ap:
        parser.error("--boundary needs --ap (Boundary AP is a second matching beside the mask AP's)")
    if not (args.dilation_ratio > 0):
        parser.error("--dilation-ratio must be > 0")
    return args


def main(argv=None):
    return run(parse_args(argv))


if __name__ == "__main__":
    main()
