"""Image-parallel dataset generation loop + the one collective of the path.

Restates the loop of ``Generate Dataset/main_sam_hbox_semantic.py:110-216`` around the drop-in
predictor: per image ``set_image`` once, ``predict_torch`` on box chunks (box-only prompt,
``multimask_output=False``), ordered painting into ``seg_mask`` (init 255, later box wins), per-box
area.  Painting / areas / class statistics run on the device (``samrs_paint``) so that only the
1 MiB class map and the per-box areas cross PCIe instead of n full-resolution masks.

``TilePipeline`` is the production loop (what ``samrs_amd.generate`` and ``bench.py`` run): batches of
tiles through ONE encoder pass, H2D of batch k+1 and decode + paint + D2H of batch k-1 overlapped with the
encoder of batch k on separate HIP streams.  ``SemanticGenerator`` is the same computation one image at a
time on one stream (the reference's shape); the two give bit-identical outputs (tests/test_pipeline_gpu.py).

Multi-GPU: images are independent, so rank r takes ``sorted(files)[r::world]`` (one process per
GPU, full weight replica) -- or, for long-tailed box counts, pulls batches of image indices from a
shared counter (``WorkQueue``) -- and there is NO collective on the data path.  The only exchange is the
dataset statistic of ``Generate Dataset/statistic.py:15-21`` -- per-class pixel and instance
counts -- which every rank accumulates locally as int64 and all-reduces once (``reduce_statistics``;
backend ``nccl`` = RCCL over xGMI on the GPU box, ``gloo`` in the CPU tests).
"""
from __future__ import annotations

import contextlib
import os

import queue
import threading
from dataclasses import dataclass, field
from typing import Callable, Iterable, Iterator, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch


def shard(items: Sequence, rank: int, world: int) -> List:
    """Static image-parallel sharding (sort first: ``os.listdir`` order is unspecified,
    main_sam_hbox_semantic.py:95)."""
    return list(sorted(items))[rank::world]


def box_chunks(n: int, batch_size: int) -> List[Tuple[int, int]]:
    """Same chunk boundaries as the reference (``part_num = n // bs + 1``; empty tail skipped,
    main_sam_hbox_semantic.py:157-181)."""
    out, start = [], 0
    end = min(n, start + batch_size)
    for _ in range(n // batch_size + 1):
        if start < end:
            out.append((start, end))
        start = end
        end = min(n, start + batch_size)
    return out


@dataclass
class ImageResult:
    seg_mask: torch.Tensor      # uint8 [H, W] on device, 255 = unlabeled
    areas: torch.Tensor         # int64 [n_boxes] on device
    masks: Optional[torch.Tensor] = None   # bool [n_boxes, H, W] when keep_masks


class SemanticGenerator:
    """hbox -> semantic label generation for one rank."""

    def __init__(self, predictor, n_classes: int, box_batch: int = 20):
        self.predictor = predictor
        self.n_classes = n_classes
        self.box_batch = box_batch
        dev = predictor.device
        self.class_pixels = torch.zeros(n_classes, dtype=torch.int64, device=dev)
        self.class_instances = torch.zeros(n_classes, dtype=torch.int64, device=dev)

    @torch.no_grad()
    def process_image(self, image: np.ndarray, boxes: np.ndarray, labels: np.ndarray, keep_masks: bool = False,
                      already_set: bool = False) -> ImageResult:
        p = self.predictor
        if not already_set:
            p.set_image(image)
        h, w = image.shape[:2]
        dev = p.device
        seg = torch.full((h, w), 255, dtype=torch.uint8, device=dev)              # :162
        gt = torch.from_numpy(np.asarray(boxes)).to(dev)
        lab = torch.from_numpy(np.asarray(labels).astype(np.int32)).to(dev)
        areas, kept = [], []
        for s, e in box_chunks(len(labels), self.box_batch):
            tb = p.transform.apply_boxes_torch(gt[s:e], (h, w))                   # :174
            masks, _, _ = p.predict_torch(None, None, tb, None, multimask_output=False)   # :176-181
            a = p.model.engine.paint(masks[:, 0], lab[s:e], seg, self.class_pixels, self.class_instances)  # :195-206
            areas.append(a)
            if keep_masks:
                kept.append(masks[:, 0])
        return ImageResult(seg, torch.cat(areas) if areas else torch.zeros(0, dtype=torch.int64, device=dev),
                           torch.cat(kept) if kept else None)


def reduce_statistics(class_pixels: torch.Tensor, class_instances: torch.Tensor, group=None):
    """SUM all-reduce of the two int64 count vectors (statistic.py:19-21 summed over all ranks).
    One message of 2*C int64 (<= 592 bytes): latency-bound, so a single fused all-reduce."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return class_pixels.clone(), class_instances.clone()
    buf = torch.cat([class_pixels, class_instances]).contiguous()
    dev = buf.device
    if dist.get_backend(group) != "nccl":            # gloo (CPU tests, ranks sharing one GPU): the message goes through the host
        buf = buf.cpu()
    dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=group)
    buf = buf.to(dev)
    c = class_pixels.numel()
    return buf[:c].clone(), buf[c:].clone()


class PolygonIoUStat:
    """One rank's running total of ``TileResult.polygon_counts`` (polygon_iou=True): the traced instances' count, their summed
    intersection and union pixels, the float64 sum of their IoUs and the smallest of them.  Instances that were not traced
    (fill = -1) are left out.  ``reduce_polygon_iou`` merges the ranks' totals."""

    def __init__(self) -> None:
        self.n, self.inter, self.union, self.total, self.low = 0, 0, 0, 0.0, float("inf")

    def add(self, counts) -> None:
        from .polygons import iou_from_counts
        c = np.asarray(counts, dtype=np.int64).reshape(-1, 3)
        c = c[c[:, 0] >= 0]
        if not len(c):
            return
        iou = iou_from_counts(c)
        self.n += len(c)
        self.inter += int(c[:, 2].sum())
        self.union += int((c[:, 0] + c[:, 1] - c[:, 2]).sum())
        self.total += float(iou.sum(dtype=np.float64))
        self.low = min(self.low, float(iou.min()))


def reduce_polygon_iou(stat: PolygonIoUStat, polygon_epsilon: float, device=None, group=None) -> dict:
    """What ``statistic/polygon_iou.json`` holds, the same on every rank: {"n": traced instances, "average": the mean of their
    IoUs, "area": sum of intersections / sum of unions, "min": the smallest IoU, "polygon_epsilon": the effective tolerance}.
    The integer sums go through ``reduce_statistics`` (the class statistics' all-reduce), the mean is a float64 SUM all-reduce over
    the ranks' sums divided by n, the minimum a MIN all-reduce.  Without a traced instance average, area and min are None; a union of
    0 pixels (every instance empty on both sides) gives area 1.0, as ``iou_from_counts`` does."""
    import torch.distributed as dist
    dev = torch.device("cpu") if device is None else device
    ints, _ = reduce_statistics(torch.tensor([stat.n, stat.inter, stat.union], dtype=torch.int64, device=dev),
                                torch.zeros(1, dtype=torch.int64, device=dev), group)
    n, inter, union = (int(v) for v in ints.cpu().tolist())
    total, low = stat.total, stat.low
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        on_dev = dist.get_backend(group) == "nccl"              # gloo: through the host, as reduce_statistics
        fsum = torch.tensor([stat.total], dtype=torch.float64, device=dev if on_dev else "cpu")
        fmin = torch.tensor([stat.low], dtype=torch.float64, device=dev if on_dev else "cpu")
        dist.all_reduce(fsum, op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(fmin, op=dist.ReduceOp.MIN, group=group)
        total, low = float(fsum.item()), float(fmin.item())
    return {"n": n, "average": total / n if n else None, "area": (inter / union if union else 1.0) if n else None,
            "min": low if n else None, "polygon_epsilon": float(polygon_epsilon)}


def agree_on_list(items: List, group=None, src: int = 0) -> List:
    """Every rank gets RANK `src`'s copy of a Python list (``broadcast_object_list``; no-op outside a process group).
    Used wherever the work list is derived from something a rank could see differently from its peers -- e.g. ``generate
    --resume`` lists the output directory while faster ranks may already be writing into it: the shards
    (``sorted(files)[r::world]``, Generate Dataset/main_sam_hbox_semantic.py:110) are only disjoint and complete when all
    ranks index the SAME list."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return list(items)
    box = [list(items) if dist.get_rank(group) == src else None]
    dist.broadcast_object_list(box, src=src, group=group)
    return box[0]


class InstancePrompter:
    """The prompt recipes of the HRSC2016 / DOTA instance drivers, one object per rank:

    * ``"point"``     -- ``Generate Dataset/main_sam_hbox_mask_instance.py:160-165``: one foreground point per object,
      ``point_coords = gt_points[:, None, :]`` passed AS IS (the reference does not run them through
      ``apply_coords``), labels all 1, no box, no mask;
    * ``"rbox_mask"`` -- ``main_sam_rbox_mask_instance.py:125-164``: the rotated box rasterised to a +-1000 mask prompt
      (``transforms.rbox_mask_prompts`` on the GPU instead of cv2), nothing else;
    * ``"box"``       -- ``main_sam_rhbox_mask_instance.py:160-168``: the enclosing horizontal box through
      ``apply_boxes_torch``.

    Boxes are processed in chunks of the engine's ``max_prompts`` (results are bit-identical to one call).
    Returns (masks bool [n, H, W], qualities fp32 [n]) on the device."""

    MODES = ("point", "rbox_mask", "box")

    def __init__(self, predictor, fill_rule: str = "auto"):
        """fill_rule: which cv2.fillPoly span rule the rbox rasteriser reproduces (transforms.resolve_fill_rule: "auto" = that of the
        cv2 installed beside this package, else the older one)."""
        from . import transforms
        self.predictor = predictor
        self.fill_rule = transforms.resolve_fill_rule(fill_rule)

    @torch.no_grad()
    def predict(self, image: np.ndarray, mode: str, hboxes=None, rboxes=None, points=None, already_set: bool = False,
                multimask_output: bool = False):
        """multimask_output=True (BASELINE.json configs[3]) decodes the three multimask outputs per object and keeps the
        one with the highest predicted IoU."""
        from . import transforms
        if mode not in self.MODES:
            raise ValueError(f"mode must be one of {self.MODES}")
        p = self.predictor
        if not already_set:
            p.set_image(image)
        h, w = image.shape[:2]
        dev = p.device
        src = {"point": points, "rbox_mask": rboxes, "box": hboxes}[mode]
        if src is None:
            raise ValueError(f"mode {mode!r} needs its annotation array")
        n = len(src)
        cap = p.model.engine.max_prompts
        masks, quals = [], []
        for s, e in box_chunks(n, cap):
            if mode == "point":
                pc = torch.as_tensor(np.asarray(points[s:e]), dtype=torch.float32, device=dev)[:, None, :]
                pl = torch.ones(e - s, 1, device=dev)
                m, q, _ = p.predict_torch(point_coords=pc, point_labels=pl, boxes=None, mask_input=None, multimask_output=multimask_output)
            elif mode == "rbox_mask":
                prompts = transforms.rbox_mask_prompts(np.asarray(rboxes[s:e]), (h, w), img_size=p.model.image_encoder.img_size,
                                                       device=dev, fill_rule=self.fill_rule)
                m, q, _ = p.predict_torch(point_coords=None, point_labels=None, boxes=None, mask_input=prompts[:, None],
                                          multimask_output=multimask_output)
            else:
                tb = p.transform.apply_boxes_torch(torch.as_tensor(np.asarray(hboxes[s:e]), dtype=torch.float32, device=dev), (h, w))
                m, q, _ = p.predict_torch(point_coords=None, point_labels=None, boxes=tb, mask_input=None, multimask_output=multimask_output)
            best = q.argmax(1) if multimask_output else torch.zeros(e - s, dtype=torch.long, device=dev)
            rows = torch.arange(e - s, device=dev)
            masks.append(m[rows, best])
            quals.append(q[rows, best])
        return torch.cat(masks), torch.cat(quals)


def mean_iou(pred_masks, gt_masks):
    """``main_sam_rhbox_mask_instance.py:222-241``: per-instance IoU averaged over the instances whose union is not empty
    ("Average mIOU"), and total intersection / total union ("Area mIOU").  Lists of [n_i, H, W] arrays, one per image."""
    ious, inter_all, union_all = [], [], []
    for pm, gm in zip(pred_masks, gt_masks):
        pm = np.asarray(pm).astype(bool)
        gm = np.asarray(gm).astype(bool)
        for j in range(pm.shape[0]):
            inter = float(np.sum(pm[j] & gm[j]))
            union = float(np.sum(pm[j] | gm[j]))
            if union > 0:
                inter_all.append(inter)
                union_all.append(union)
                ious.append(inter / union)
    if not ious:
        return float("nan"), float("nan")
    return float(np.mean(ious)), float(np.sum(inter_all) / np.sum(union_all))


# ------------------------------------------------------------------------------------------------
# Work distribution across ranks
# ------------------------------------------------------------------------------------------------
class WorkQueue:
    """Hands out consecutive index ranges [start, end) of a sorted work list to the ranks of one job.

    * ``mode="static"``  -- rank r owns the chunks r, r + world, r + 2 world, ... (no communication; with
      ``chunk=1`` this is ``sorted(files)[r::world]``);
    * ``mode="dynamic"`` -- a shared counter: every pull is one atomic fetch-add of ``chunk`` on the job's
      rendezvous store (``torch.distributed`` TCPStore ``add``: one small round trip to rank 0's store thread,
      ~0.1 ms, against ~60 ms of GPU work per 8-tile chunk).  A rank that drew images with hundreds of boxes
      (DOTA-v2: a few per cent of the tiles) simply pulls less often, so the 8 GPUs finish together instead
      of waiting for the unluckiest static shard.  The data path itself still has no collective.
    """

    _seq = 0          # queues created by this process: every rank creates its queues in the same order

    def __init__(self, n_items: int, chunk: int = 1, rank: int = 0, world: int = 1, mode: str = "static",
                 store=None, name: Optional[str] = None):
        """`name` keys the shared counter on the store: it must be the same on every rank and UNIQUE per work list (a spent
        counter would hand a second queue of the same name nothing).  Default: a per-process sequence number."""
        if mode not in ("static", "dynamic"):
            raise ValueError("mode must be 'static' or 'dynamic'")
        if name is None:
            name = f"samrs_wq/{WorkQueue._seq}"
        WorkQueue._seq += 1
        self.n, self.chunk, self.rank, self.world, self.mode = int(n_items), int(chunk), rank, world, mode
        self._k = 0
        self._local = 0
        self._key = name + "/head"
        self._store = None
        if mode == "dynamic" and world > 1:
            if store is None:
                import torch.distributed as dist
                from torch.distributed.distributed_c10d import _get_default_store
                if not dist.is_initialized():
                    raise RuntimeError("dynamic WorkQueue over several ranks needs an initialised process group (its store)")
                store = _get_default_store()
            self._store = store

    def pull(self) -> Optional[Tuple[int, int]]:
        """Next range, or None when the list is exhausted."""
        if self.mode == "static":
            start = (self._k * self.world + self.rank) * self.chunk
            self._k += 1
        elif self._store is None:
            start = self._local
            self._local += self.chunk
        else:
            start = int(self._store.add(self._key, self.chunk)) - self.chunk
        if start >= self.n:
            return None
        return start, min(self.n, start + self.chunk)

    def __iter__(self) -> Iterator[Tuple[int, int]]:
        while True:
            r = self.pull()
            if r is None:
                return
            yield r


def gather_mask_sizes(local_sizes: Sequence[int], group=None) -> List[int]:
    """All ranks' per-instance mask sizes in rank order -- the list `Generate Dataset/statistic.py:34-53` builds from
    every ``ins/*.pkl`` (``all_mask_size``).  Variable length per rank: all-gather of the counts, then of the
    sizes padded to the longest rank (RCCL on the GPU box, gloo in the CPU tests)."""
    import torch.distributed as dist
    sizes = torch.as_tensor(list(local_sizes), dtype=torch.int64)
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return sizes.tolist()
    world = dist.get_world_size(group)
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
    cnt = torch.tensor([sizes.numel()], dtype=torch.int64, device=dev)
    counts = [torch.zeros_like(cnt) for _ in range(world)]
    dist.all_gather(counts, cnt, group=group)
    m = max(int(c.item()) for c in counts)
    buf = torch.zeros(max(m, 1), dtype=torch.int64, device=dev)
    buf[: sizes.numel()] = sizes.to(dev)
    bufs = [torch.zeros_like(buf) for _ in range(world)]
    dist.all_gather(bufs, buf, group=group)
    out: List[int] = []
    for c, b in zip(counts, bufs):
        out.extend(b[: int(c.item())].cpu().tolist())
    return out


# ------------------------------------------------------------------------------------------------
# The production loop
# ------------------------------------------------------------------------------------------------
@dataclass
class WorkItem:
    """One image of the stream: uint8 HWC pixels (host numpy array, host tensor or device tensor), its boxes in
    ORIGINAL-image pixels (xyxy) and their class labels; `key` travels to the sink untouched.  `gt` (only read by
    ``InstancePipeline(gt=True)``): ``(label_rgb, colors)``, the host label image uint8 [H, W, 3] and one colour uint8 [3] per
    annotation -- instance j's ground truth is the label pixels of colour j (main_sam_rhbox_mask_instance.py:210-214)."""
    key: object
    image: object
    boxes: np.ndarray
    labels: np.ndarray
    gt: Optional[Tuple[np.ndarray, np.ndarray]] = None


@dataclass
class TileResult:
    key: object
    seg_mask: np.ndarray                    # uint8 [H, W] host, 255 = unlabeled (a view of a pinned ring buffer)
    areas: np.ndarray                       # int64 [n_boxes] host
    boxes: np.ndarray
    labels: np.ndarray
    masks: Optional[np.ndarray] = None      # uint8 [n_boxes, H, W] host when keep_masks
    quality: Optional[np.ndarray] = None    # fp32 [n_boxes] predicted IoU of the kept mask (instance pipelines; TilePipeline(quality=True))
    rle_table: Optional[np.ndarray] = None  # int64 [n_boxes, 3] (offset, length, n_counts) into rle_data when rle=True
    rle_data: Optional[np.ndarray] = None   # uint8 view of the batch's pinned RLE byte buffer
    size: Optional[Tuple[int, int]] = None  # (H, W) of the tile
    inter: Optional[np.ndarray] = None      # int64 [n_boxes] |mask AND ground truth| (InstancePipeline(gt=True))
    gt_area: Optional[np.ndarray] = None    # int64 [n_boxes] |ground truth| (InstancePipeline(gt=True))
    gt_rle_table: Optional[np.ndarray] = None   # like rle_table, for the ground-truth masks (gt=True, rle=True)
    gt_rle_data: Optional[np.ndarray] = None
    png_table: Optional[np.ndarray] = None  # int64 [2, 2] (offset, length) of the gray and the colour PNG in png_data (png_lut)
    png_data: Optional[np.ndarray] = None   # uint8 view of the batch's pinned PNG byte buffer
    vis_table: Optional[np.ndarray] = None  # int64 [2] (offset, length) of the overlay PNG in vis_data (vis_lut)
    vis_data: Optional[np.ndarray] = None   # uint8 view of the batch's pinned overlay byte buffer
    changed: Optional[np.ndarray] = None    # int64 [n_boxes] pixels the small-region clean-up changed (min_region_area > 0)
    removed: Optional[np.ndarray] = None    # int64 [n_boxes] pixels the overlap stage took from the instance (overlap != "order")
    # mask_boxes=True (samrs_mask_boxes, in the image's own frame; an empty mask has mask_record[j, 6] == 0 and zeros everywhere):
    mask_hbox: Optional[np.ndarray] = None  # int32 [n_boxes, 4] xmin, ymin, xmax, ymax (inclusive) of the set pixels
    mask_rbox: Optional[np.ndarray] = None  # fp32 [n_boxes, 4, 2] corners of the minimum-area rotated rectangle of the pixel centres
    mask_record: Optional[np.ndarray] = None    # int64 [n_boxes, 8] dx, dy, pmin, pmax, qmin, qmax, hull vertices m, 2 x hull area
    gt_hbox: Optional[np.ndarray] = None    # int32 [n_boxes, 4] the same hbox of the ground-truth masks (gt=True, rle=True, mask_boxes=True)
    # TilePipeline(quality=True) (samrs_score_masks / samrs_filter_masks; helpers in samrs_amd/quality.py):
    score_counts: Optional[np.ndarray] = None   # int64 [n_boxes, 4] pixels with logit > +1, > 0, > -1, and > 0 inside the prompt box
    kept: Optional[np.ndarray] = None       # bool [n_boxes] the instance passed the thresholds (all true without thresholds)
    # polygons=True (samrs_mask_polygons; vertices are corners of the pixel lattice, in the image's / scene's own frame):
    polygon_table: Optional[np.ndarray] = None      # int64 [n_boxes, 5] first ring, ring count, first vertex, vertex count, edge count
    polygon_rings: Optional[np.ndarray] = None      # int32 [R, 4] the batch's ring records (the table's firsts index them)
    polygon_vertices: Optional[np.ndarray] = None   # int32 [V, 2] the batch's vertices
    # polygon_iou=True (samrs_fill_polygons on the rings as they are handed out, against the mask they were traced from):
    polygon_counts: Optional[np.ndarray] = None     # int64 [n_boxes, 3] pixels of the rings' fill (-1: not traced), of the mask, of both
    # InstancePipeline(gt=True, ap=True) (samrs_coco_match on every prediction x every ground truth of the tile; per tile, not per box):
    ap_order: Optional[np.ndarray] = None       # int32 [100] detection index per rank (score descending, stable), -1 past n_kept
    ap_match: Optional[np.ndarray] = None       # int32 [4, 10, 100] matched ground-truth INDEX per area range, IoU threshold and rank, -1 = none
    ap_dt_ignore: Optional[np.ndarray] = None   # uint8 [4, 10, 100] the detection does not count at that range / threshold
    ap_n_valid: Optional[np.ndarray] = None     # int32 [4] ground truths inside each area range
    ap_n_kept: Optional[np.ndarray] = None      # int32 [1] ranks in use = min(n_boxes, 100)
    # InstancePipeline(gt=True, ap=True, boundary=True): the same matching on min(mask IoU, boundary IoU) (samrs_coco_match_min) ...
    boundary_order: Optional[np.ndarray] = None     # int32 [100], as ap_order (the scores are the same, so it equals ap_order)
    boundary_match: Optional[np.ndarray] = None     # int32 [4, 10, 100], as ap_match
    boundary_dt_ignore: Optional[np.ndarray] = None # uint8 [4, 10, 100], as ap_dt_ignore
    boundary_n_valid: Optional[np.ndarray] = None   # int32 [4], as ap_n_valid (the area ranges look at the MASK areas)
    boundary_n_kept: Optional[np.ndarray] = None    # int32 [1], as ap_n_kept
    # ... and per object the diagonal of the band counts, for the Boundary mIoU (union = band_area_d + band_area_g - band_inter):
    band_inter: Optional[np.ndarray] = None     # int64 [n_boxes] |band(kept mask j) AND band(ground truth j)|
    band_area_d: Optional[np.ndarray] = None    # int64 [n_boxes] |band(kept mask j)|
    band_area_g: Optional[np.ndarray] = None    # int64 [n_boxes] |band(ground truth j)|
    windows: Optional[List[Tuple[int, int, int, int]]] = None   # scene mode (scene.ScenePipeline): the planned (x0, y0, w, h) windows
    window_of: Optional[List[int]] = None   # scene mode: window_of[j] = index into `windows` of the window box j was decoded in

    @property
    def ap_tables(self) -> Optional[dict]:
        """This tile's COCO matching as ``coco_ap.accumulate`` takes it (scores = `quality`, order, match, dt_ignore, n_valid,
        n_kept); None unless the pipeline ran with ap=True."""
        if self.ap_order is None:
            return None
        return {"scores": np.asarray(self.quality, dtype=np.float64), "order": self.ap_order, "match": self.ap_match,
                "dt_ignore": self.ap_dt_ignore, "n_valid": self.ap_n_valid, "n_kept": int(self.ap_n_kept[0])}

    @property
    def boundary_tables(self) -> Optional[dict]:
        """This tile's Boundary AP matching, shaped like ``ap_tables``, plus the per-object band counts band_inter, band_area_d and
        band_area_g (int64 [n_boxes]); None unless the pipeline ran with boundary=True."""
        if self.boundary_order is None:
            return None
        return {"scores": np.asarray(self.quality, dtype=np.float64), "order": self.boundary_order, "match": self.boundary_match,
                "dt_ignore": self.boundary_dt_ignore, "n_valid": self.boundary_n_valid, "n_kept": int(self.boundary_n_kept[0]),
                "band_inter": self.band_inter, "band_area_d": self.band_area_d, "band_area_g": self.band_area_g}

    def png(self, kind: str) -> memoryview:
        """The bytes of ``gray/<stem>.png`` (kind "gray") or ``color/<stem>.png`` ("color") of this tile, encoded on the device
        (samrs_png_encode_labels) and byte-identical with tile_io.write_label_pair; only when the pipeline ran with png_lut.
        Kind "vis": the bytes of ``vis/<stem>.png``, visualize.py's blend of the image with this class map through the pipeline's
        vis_lut (samrs_blend_labels, samrs_png_encode_rgb); only when the pipeline ran with vis_lut."""
        if kind == "vis":
            if self.vis_table is None:
                raise ValueError("no overlay PNG file: the pipeline ran without vis_lut")
            off, n = (int(v) for v in self.vis_table)
            return memoryview(self.vis_data[off:off + n])
        if self.png_table is None:
            raise ValueError("no device PNG files: the pipeline ran without png_lut")
        off, n = (int(v) for v in self.png_table[{"gray": 0, "color": 1}[kind]])
        return memoryview(self.png_data[off:off + n])

    def mask_bbox(self, j: int) -> Optional[List[int]]:
        """COCO ``[x, y, w, h]`` of instance j's mask (w = xmax - xmin + 1: whole pixels), None for an empty mask."""
        if int(self.mask_record[j, 6]) == 0:
            return None
        x0, y0, x1, y1 = (int(v) for v in self.mask_hbox[j])
        return [x0, y0, x1 - x0 + 1, y1 - y0 + 1]

    def polygons(self, j: int) -> Optional[list]:
        """Instance j's outline as a list of (int32 [k, 2] lattice vertices, is_hole), outer rings and holes in the library's order
        (``samrs_amd.polygons.rings_of``; ``polygons.nest`` groups them); [] for an empty or dropped mask, None for a mask with more
        edges than the pipeline's polygon_max_edges (not traced; polygon_table[j, 4] holds its edge count)."""
        from .polygons import rings_of
        return rings_of(self.polygon_table, self.polygon_rings, self.polygon_vertices, j)

    def polygon_iou(self, j: int) -> Optional[float]:
        """IoU of instance j's mask with the even-odd fill of the rings ``polygons(j)`` hands out (what `polygon_epsilon` cost; exactly
        1.0 without it): ``polygons.iou_from_counts(polygon_counts[j])``; None where the mask was not traced.  Only when the
        pipeline ran with polygon_iou=True."""
        from .polygons import iou_from_counts
        if self.polygon_counts is None:
            raise ValueError("no polygon counts: the pipeline ran without polygon_iou")
        return None if int(self.polygon_counts[j, 0]) < 0 else float(iou_from_counts(self.polygon_counts[j]))

    def rle(self, j: int) -> dict:
        """COCO RLE of instance j exactly as the reference stores it (main_sam_hbox_semantic.py:201-202):
        ``{"size": [H, W], "counts": str}``; encoded on the device (samrs_rle_encode)."""
        off, n, _ = (int(v) for v in self.rle_table[j])
        return {"size": [int(self.size[0]), int(self.size[1])], "counts": self.rle_data[off:off + n].tobytes().decode("ascii")}

    def gt_rle(self, j: int) -> Optional[dict]:
        """COCO RLE of instance j's ground-truth mask (instance_to_json.py:44-45), encoded on the device; None unless the
        pipeline ran with gt=True and rle=True."""
        if self.gt_rle_table is None:
            return None
        off, n, _ = (int(v) for v in self.gt_rle_table[j])
        return {"size": [int(self.size[0]), int(self.size[1])], "counts": self.gt_rle_data[off:off + n].tobytes().decode("ascii")}


class OutputTable(NamedTuple):
    """One fixed-size per-box output, declared once (``output_tables``): per input set a device table [batch, max_boxes, *tail] that
    the decode chain fills, per output buffer a pinned mirror, per tile the ``TileResult`` field of its [n_boxes, *tail] rows.
    A `per_tile` output has one row per tile instead: tables [batch, *tail], the field is the tile's whole row."""
    field: str                      # the TileResult field
    dev: str                        # the pipeline attribute that holds the two device tables
    tail: Tuple[int, ...]           # shape of one box's row
    dtype: torch.dtype
    fill: Optional[str] = "zeros"   # the device tables start as "zeros" / "ones" / None: uninitialised
    as_bool: bool = False           # the host rows: a copy, or astype(bool)
    per_tile: bool = False          # one row per tile, not per box: the tables are [batch, *tail] and a tile's result is its whole row

    def alloc(self, batch: int, max_boxes: int, device=None) -> torch.Tensor:
        """The device table (filled) on `device`; without one, its pinned host mirror."""
        shape = (batch, *self.tail) if self.per_tile else (batch, max_boxes, *self.tail)
        if device is None:
            return torch.empty(shape, dtype=self.dtype).pin_memory()
        return {"zeros": torch.zeros, "ones": torch.ones, None: torch.empty}[self.fill](shape, dtype=self.dtype, device=device)

    def rows(self, host: torch.Tensor) -> np.ndarray:
        a = host.numpy()
        return a.astype(bool) if self.as_bool else a.copy()


def output_tables(min_region_area: int = 0, mask_boxes: bool = False, quality: bool = False, gt: bool = False, rle: bool = False,
                  instance: bool = False, overlap: str = "order", ap: bool = False, boundary: bool = False,
                  polygon_iou: bool = False) -> List[OutputTable]:
    """The per-box tables a pipeline with these (resolved) options allocates, copies to the host and hands out, in that order.
    Pure.  An option that is off contributes nothing: no allocation, no copy, and its TileResult fields stay None.  `instance`: an
    InstancePipeline, which always reports the predicted IoU of the mask it kept.  `ap`: the per-tile tables of the COCO matching
    (``AP_SHAPE`` = area ranges, IoU thresholds, max detections); `boundary`: a second set of them for the matching on min(mask IoU,
    boundary IoU), and per box the diagonal band counts.  `polygon_iou`: per box the three counts of ``Engine.fill_polygons``."""
    T, i64, i32 = OutputTable, torch.int64, torch.int32
    tabs = [T("areas", "area_dev", (), i64)]
    if min_region_area:
        tabs.append(T("changed", "chg_dev", (), i64))
    if overlap != "order":
        tabs.append(T("removed", "rem_dev", (), i64))
    if mask_boxes:
        tabs += [T("mask_hbox", "hbox_dev", (4,), i32), T("mask_rbox", "rbox_dev", (4, 2), torch.float32),
                 T("mask_record", "rec_dev", (8,), i64)]
    if quality:
        tabs += [T("score_counts", "cnt_dev", (4,), i64), T("kept", "keep_dev", (), torch.uint8, "ones", True)]
    if quality or instance:
        tabs.append(T("quality", "qual_dev", (), torch.float32))
    if gt:
        tabs += [T("inter", "inter_dev", (), i64), T("gt_area", "gta_dev", (), i64)]
        if rle and mask_boxes:      # the ground-truth masks are only materialised for their RLE
            tabs.append(T("gt_hbox", "gt_hbox_dev", (4,), i32))
    if ap:
        A, Tn, D = AP_SHAPE
        tile = dict(fill=None, per_tile=True)       # every tile's row is written whole by samrs_coco_match
        tabs += [T("ap_order", "ap_order_dev", (D,), i32, **tile), T("ap_match", "ap_match_dev", (A, Tn, D), i32, **tile),
                 T("ap_dt_ignore", "ap_ign_dev", (A, Tn, D), torch.uint8, **tile), T("ap_n_valid", "ap_nvalid_dev", (A,), i32, **tile),
                 T("ap_n_kept", "ap_nkept_dev", (1,), i32, **tile)]
    if boundary:
        A, Tn, D = AP_SHAPE
        tile = dict(fill=None, per_tile=True)       # written whole by samrs_coco_match_min
        tabs += [T("boundary_order", "bd_order_dev", (D,), i32, **tile), T("boundary_match", "bd_match_dev", (A, Tn, D), i32, **tile),
                 T("boundary_dt_ignore", "bd_ign_dev", (A, Tn, D), torch.uint8, **tile),
                 T("boundary_n_valid", "bd_nvalid_dev", (A,), i32, **tile), T("boundary_n_kept", "bd_nkept_dev", (1,), i32, **tile),
                 T("band_inter", "band_inter_dev", (), i64), T("band_area_d", "band_ad_dev", (), i64),
                 T("band_area_g", "band_ag_dev", (), i64)]
    if polygon_iou:
        tabs.append(T("polygon_counts", "pcnt_dev", (3,), i64))
    return tabs


AP_SHAPE = (4, 10, 100)     # coco_ap.AREA_RANGES, IOU_THRESHOLDS, MAX_DETS[-1]


def check_packed(tab: np.ndarray, total: int, holder: str, now: int, what: str = "RLE buffer too small: a mask",
                 knob: str = "rle_buffer_mb") -> None:
    """Raises for a packed string table (rows of (offset, length, ...)) with an entry that did not fit: its length is
    -1 - the bytes it needs.  `holder`: "batch" / "scene", whatever shares the buffer; `now`: the buffer's size in MiB."""
    if len(tab) and int(tab[:, 1].min()) < 0:
        raise RuntimeError(f"{what} needs {int((-tab[:, 1] - 1).max())} bytes and the {holder} already holds {total}; raise "
                           f"{knob} (now {now})")


def check_polygons(tab: np.ndarray, nv: int, nr: int, holder: str, now: int) -> None:
    """Raises for a polygon table with a mask that did not fit (ring count -1 - rings needed, vertex count -1 - vertices needed);
    a mask over the edge cap stays (-1, -1)."""
    if len(tab) and int(tab[:, 1].min()) < -1:
        j = int(np.argmin(tab[:, 1]))
        raise RuntimeError(f"polygon buffer too small: a mask needs {int(-tab[j, 3] - 1)} vertices and {int(-tab[j, 1] - 1)} rings and "
                           f"the {holder} already holds {nv} and {nr}; raise polygon_buffer_mb (now {now})")


OVERLAP_OPTIONS = ("order", "logit", "smallest")       # TilePipeline(overlap=...): "order" = painting order, nothing launched


def polygon_eps_q(polygon_epsilon: float = 0.0, polygons: bool = True) -> int:
    """The one declaration of the `polygon_epsilon` option: what the pipelines' argument becomes -- the tolerance of
    ``Engine.simplify_polygons`` in sixteenths of a pixel, round(16 * polygon_epsilon), or 0 = off (no call is made).  It needs
    polygons=True, must be >= 0 and at most 1024 pixels (eps_q <= 16384); a positive value below 1/32 pixel rounds to no tolerance at
    all and is refused.  The effective tolerance is eps_q / 16.  Pure."""
    from .engine import POLYGON_EPS_Q_MAX
    eps = float(polygon_epsilon)
    if eps != eps or eps < 0:
        raise ValueError(f"polygon_epsilon must be >= 0 (0 = off), got {polygon_epsilon!r}")
    if eps == 0:
        return 0
    if not polygons:
        raise ValueError("polygon_epsilon simplifies the traced polygons: it needs polygons=True")
    q = int(round(16.0 * min(eps, 1e6)))
    if q > POLYGON_EPS_Q_MAX:
        raise ValueError(f"polygon_epsilon = {polygon_epsilon!r} is above {POLYGON_EPS_Q_MAX // 16} pixels (eps_q = {q} > {POLYGON_EPS_Q_MAX})")
    if q < 1:
        raise ValueError(f"polygon_epsilon = {polygon_epsilon!r} rounds to 0 sixteenths of a pixel: pass 0 (off) or at least 1 / 32")
    return q


def validate_output_options(min_region_area: int = 0, region_mode: str = "both", polygons: bool = False, polygon_buffer_mb: int = 64,
                            polygon_max_edges: int = 65536, png_lut=None, overlap: str = "order", polygon_epsilon: float = 0.0,
                            polygon_iou: bool = False):
    """The output options TilePipeline and ScenePipeline share, checked in one place -> (png_lut as contiguous uint8 [256, 3] or
    None, the vertices one polygon buffer holds or None).  `overlap` is TilePipeline's alone (ScenePipeline refuses it before it gets
    here: ``refuse_overlap_option``).  `polygon_epsilon` is checked here and resolved by ``polygon_eps_q``.  `polygon_iou` (the rings filled again on the device
    and counted against their mask) needs polygons=True; ScenePipeline and InstancePipeline refuse it (``refuse_polygon_iou_option``).
    Touches no device."""
    from .engine import REGION_MODES
    polygon_eps_q(polygon_epsilon, bool(polygons))
    if polygon_iou and not polygons:
        raise ValueError("polygon_iou scores the traced polygons against their masks: it needs polygons=True")
    if overlap not in OVERLAP_OPTIONS:
        raise ValueError(f"overlap must be one of {list(OVERLAP_OPTIONS)}, got {overlap!r}")
    if int(min_region_area) < 0:
        raise ValueError("min_region_area must be >= 0 (0 = off)")
    if region_mode not in REGION_MODES:
        raise ValueError(f"region_mode must be one of {sorted(REGION_MODES)}, got {region_mode!r}")
    lut = nv = None
    if png_lut is not None:
        lut = np.ascontiguousarray(png_lut, dtype=np.uint8)
        if lut.shape != (256, 3):
            raise ValueError("png_lut must be uint8 [256, 3] (tile_io.class_lut)")
    if polygons:
        if int(polygon_buffer_mb) < 1 or int(polygon_max_edges) < 4:
            raise ValueError("polygon_buffer_mb must be >= 1 and polygon_max_edges >= 4")
        nv = (int(polygon_buffer_mb) << 20) // 12              # 8 bytes per vertex + 16 per ring, a ring has >= 4 vertices
    return lut, nv


class PackedStream:
    """One variable-length output of a batch, packed on the device behind a cursor (samrs_rle_encode's layout).  Per input set:
    the payload buffers, a cursor (int64, one count of rows used per payload) and a table of `rows` x `tail` int64 that says where
    each entry lies.  Per output buffer (``pinned``): mirrors of the table and the cursor, and payloads that grow on demand.
    The device payloads are attributes of the pipeline, two tensors each, named in `payloads` as (attribute, row tail, dtype, pinned
    rows to begin with) and read at each use.  `check(table, used)` raises for a table with an entry that did not fit.
    RLE, ground-truth RLE and PNG have one byte payload; polygons have two (vertices, ring records) and fit without a special case."""

    def __init__(self, pipe, name: str, rows: int, tail: Tuple[int, ...], payloads, check):
        self.pipe, self.name, self.shape, self.payloads, self.check = pipe, name, (rows, *tail), payloads, check
        self.cur = [torch.zeros(len(payloads), dtype=torch.int64, device=pipe.dev) for _ in range(2)]
        self.tab = [torch.zeros(self.shape, dtype=torch.int64, device=pipe.dev) for _ in range(2)]

    def pinned(self) -> list:
        """[table, cursor, [payloads]] on the host, for one _OutBuf."""
        return [torch.zeros(self.shape, dtype=torch.int64).pin_memory(), torch.zeros(len(self.payloads), dtype=torch.int64).pin_memory(),
                [torch.empty(n, *tail, dtype=dtype).pin_memory() for _, tail, dtype, n in self.payloads]]

    def reset(self, b: int) -> None:
        self.cur[b].zero_()

    def copy_table(self, b: int, out: "_OutBuf") -> None:
        tab, cur, _ = out.packed[self.name]
        tab.copy_(self.tab[b], non_blocking=True)
        cur.copy_(self.cur[b], non_blocking=True)

    def fetch(self, b: int, out: "_OutBuf", n: int):
        """(the first n table rows, the pinned payloads, the rows used of each) of a batch whose table and cursor are on the host
        (out.done), so the payloads can be copied with their exact size -- on a copy stream, while the GPU works on the batches
        already queued."""
        tab, cur, host = out.packed[self.name]
        tab = tab.view(-1, tab.shape[-1])[:n].numpy()
        used = cur.tolist()
        self.check(tab, used)
        for k, (_, tail, dtype, _) in enumerate(self.payloads):
            if host[k].shape[0] < used[k]:
                host[k] = torch.empty(max(used[k], 2 * host[k].shape[0]), *tail, dtype=dtype).pin_memory()
        if any(used):
            with torch.cuda.stream(self.pipe.s_d2h):
                for k, (attr, _, _, _) in enumerate(self.payloads):
                    host[k][:used[k]].copy_(getattr(self.pipe, attr)[b][:used[k]], non_blocking=True)
            self.pipe.s_d2h.synchronize()
        return tab, host, used


class _OutBuf:
    """One batch's results in pinned host memory: the class maps, a mirror of each active per-box table (by TileResult field) and
    of each packed stream (by its name)."""

    def __init__(self, batch: int, side: int, max_boxes: int, tables: Sequence[OutputTable], streams: Sequence[PackedStream] = ()):
        self.seg = torch.empty(batch, side, side, dtype=torch.uint8).pin_memory()
        self.tables = {t.field: t.alloc(batch, max_boxes) for t in tables}
        self.packed = {s.name: s.pinned() for s in streams}
        self.done = torch.cuda.Event()
        self.masks: List[Optional[torch.Tensor]] = [None] * batch     # keep_masks: host copies of the full masks
        self.odd: dict = {}                                           # tiles that are not side x side: their class maps


QUALITY_OPTIONS = ("quality", "min_stability", "min_pred_iou", "min_inside_box")


def refuse_quality_options(who: str, why: str, **opts) -> None:
    """ValueError naming the mask-quality options of TilePipeline that `who` was handed (a pipeline that does not score masks)."""
    given = [k for k in QUALITY_OPTIONS if opts.get(k)]
    if given:
        raise ValueError(f"{who} does not score masks ({why}): {', '.join(given)} "
                         f"{'is a' if len(given) == 1 else 'are'} TilePipeline option{'' if len(given) == 1 else 's'}")


def refuse_vis_option(who: str, why: str, **opts) -> None:
    """ValueError naming TilePipeline's `vis_lut` option when `who` (a pipeline that writes no overlays) was handed one."""
    if opts.get("vis_lut") is not None:
        raise ValueError(f"{who} writes no overlays ({why}): vis_lut is a TilePipeline option")


def validate_vis_options(vis_lut, vis_alpha: float = 0.4, vis_buffer_mb: Optional[int] = None):
    """TilePipeline's overlay options -> (vis_lut as contiguous uint8 [256, 3], alpha), or (None, alpha) without vis_lut.
    Touches no device."""
    if vis_lut is None:
        return None, float(vis_alpha)
    lut = np.ascontiguousarray(vis_lut, dtype=np.uint8)
    if lut.shape != (256, 3):
        raise ValueError("vis_lut must be uint8 [256, 3] (tile_io.class_lut)")
    alpha = float(vis_alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"vis_alpha must lie in [0, 1], got {vis_alpha!r}")
    if vis_buffer_mb is not None and int(vis_buffer_mb) < 1:
        raise ValueError("vis_buffer_mb must be >= 1")
    return lut, alpha


def refuse_boundary_option(who: str, why: str, **opts) -> None:
    """ValueError naming InstancePipeline's `boundary` option when `who` (a pipeline without ground truth to match against) was handed it."""
    if opts.get("boundary"):
        raise ValueError(f"{who} evaluates nothing against ground truth ({why}): boundary is an InstancePipeline option "
                         f"(gt=True, ap=True, boundary=True)")


def refuse_polygon_iou_option(who: str, why: str, **opts) -> None:
    """ValueError naming TilePipeline's `polygon_iou` option when `who` (a pipeline that does not score polygons against their masks)
    was handed it."""
    if opts.get("polygon_iou"):
        raise ValueError(f"{who} does not score polygons against their masks ({why}): polygon_iou is a TilePipeline option")


def refuse_overlap_option(who: str, why: str, **opts) -> None:
    """ValueError naming TilePipeline's `overlap` option when `who` (a pipeline that does not resolve overlapping masks) was handed
    anything but "order"."""
    value = opts.get("overlap", "order")
    if value != "order":
        raise ValueError(f"{who} does not resolve overlapping masks ({why}): overlap={value!r} is a TilePipeline option")


DECODE_PROMPTS_LIMIT = 512      # the engine's cap on option "decode_prompts" (samrs_hip.h)


def resolve_batch_decode(batch_decode, batch: int, box_batch: int, max_boxes: int, max_prompts: int, max_images: int,
                         capacity: int) -> Tuple[bool, Optional[int], str]:
    """What a pipeline's ``batch_decode`` argument becomes: (on, the "decode_prompts" to ask the engine for or None, why).  Pure.

    True / False stand as they are and ask for nothing.  "auto" is on when
      * box_batch >= max_boxes: no tile is decoded in several chunks (the c2 / c4 shape).  A long-tailed batch (c3: up to 400 boxes
        in 64-box chunks) keeps the per-tile chains it has; nothing was measured to gain there; and
      * one chain holds the whole batch, batch x max_boxes prompts: the engine's capacity as it stands (`capacity`), or a value it
        accepts -- [max_prompts, min(max_images x max_prompts, DECODE_PROMPTS_LIMIT)] -- which is then the value to set.
    No output option is part of the rule: min_region_area, quality, mask_boxes and polygons give byte for byte the same outputs
    under batch_decode=True as without it (tests/test_clean_masks_gpu.py, test_quality_gpu.py, test_polygons_gpu.py)."""
    if batch_decode != "auto":
        return bool(batch_decode), None, "explicit"
    if box_batch < max_boxes:
        return False, None, f"box_batch={box_batch} < max_boxes={max_boxes}: tiles are decoded in several chunks"
    need = batch * max_boxes
    if need <= capacity:
        return True, None, f"a chain of {need} prompts fits the engine's decode_prompts={capacity}"
    hi = min(max_images * max_prompts, DECODE_PROMPTS_LIMIT)
    if need > hi:
        return False, None, f"a chain of {need} prompts exceeds what the engine accepts ({hi})"
    return True, need, f"decode_prompts raised from {capacity} to {need}"


class TilePipeline:
    """hbox -> semantic labels for a stream of tiles (main_sam_hbox_semantic.py:110-216), restructured for the GPU:

        stream h2d : pinned staging -> HBM            tiles + boxes of batch k+1
        stream enc : samrs_set_images(_ragged)        batch k   (one encoder pass over `batch` tiles)
        stream dec : predict (box chunks) + paint     batch k-1 (reads the OTHER embedding slot set)
                     + D2H of class maps / areas
        host       : hands batch k-2 to `sink`        (PNG / pickle writers run in a thread pool there)

    Two embedding slot sets and two input staging sets, `out_depth` pinned output buffers.  What crosses PCIe per
    tile: 3 MiB in, 1 MiB class map + 8 B per box out (`samrs_paint` runs on the device), and with `rle=True` the
    per-instance COCO RLE strings of main_sam_hbox_semantic.py:201-202, encoded on the device (`samrs_rle_encode`:
    a few KB per mask on real data) -- the full-resolution masks themselves never leave HBM unless `keep_masks`.  Bit-identical to `SemanticGenerator` (no kernel depends on batch composition or on what
    runs next to it).  Tiles of one batch may differ in size (non-1024 tiles are resized on the GPU, bit-exact with
    PIL, and encoded through samrs_set_images_ragged).

    With `png_lut` (uint8 [256, 3], ``tile_io.class_lut(palette)``) the class maps are also encoded on the device into the
    complete ``gray/<stem>.png`` and ``color/<stem>.png`` files (`samrs_png_encode_labels`, byte-identical with
    ``tile_io.write_label_pair``): ``TileResult.png(kind)``.  `png_buffer_mb` is the device buffer for one batch's files
    (default: 6 MiB per tile, which holds a batch of all-literal 1024^2 tiles -- at most 9 bits per byte, 4.5 MiB per pair).

    With `vis_lut` (uint8 [256, 3]) every tile also yields visualize.py's overlay, ``Image.blend(image, vis_lut[seg_mask],
    vis_alpha)`` bit for bit, as a complete truecolour PNG file: ``TileResult.png("vis")``.  The blend (`samrs_blend_labels`) runs
    on the decode stream after painting, at the image's own size and from its original pixels (an odd-sized tile blends the
    uploaded original, not the resized tile), and `samrs_png_encode_rgb` packs the files into a buffer of their own.
    `vis_buffer_mb` is that buffer for one batch (default: the encoder's documented worst case for a batch of side x side tiles,
    ``engine.png_rgb_bound``); a batch that overflows it raises, naming the option.  Input set b is then read after the encoder,
    so it is handed back to staging only once the batch's blends are enqueued.  None (default) launches and allocates nothing,
    and event order, allocations and results are what they were."""

    BOX_WIDTH = 4          # floats per annotation: xyxy

    def __init__(self, sam, n_classes: int, batch: int = 8, box_batch: int = 20, keep_masks: bool = False,
                 out_depth: int = 3, max_boxes: int = 512, device_inputs: bool = False, rle: bool = False,
                 rle_buffer_mb: int = 256, precision="auto", _multimask: bool = False, png_lut: Optional[np.ndarray] = None,
                 png_buffer_mb: Optional[int] = None, batch_decode="auto", min_region_area: int = 0,
                 region_mode: str = "both", mask_boxes: bool = False, quality: bool = False, min_stability: float = 0.0,
                 min_pred_iou: float = 0.0, min_inside_box: float = 0.0, polygons: bool = False, polygon_buffer_mb: int = 64,
                 polygon_max_edges: int = 65536, overlap: str = "order", vis_lut: Optional[np.ndarray] = None, vis_alpha: float = 0.4,
                 vis_buffer_mb: Optional[int] = None, boundary: bool = False, polygon_epsilon: float = 0.0, polygon_iou: bool = False):
        """precision: the operand-split mode (engine option "split") THIS PIPELINE'S OWN CALLS run in.  The option is set around
        each of the pipeline's encode / decode calls and restored afterwards (``Engine.options``), so the mode never outlives
        them: a ``SamPredictor`` built on the same model keeps the engine's own default (round 3 changed the engine's option for
        good, and whoever built the last pipeline decided everybody's precision).  The mode an image was encoded in is
        recorded with its embedding slot (``Engine.get_slot_info``).
        "auto" = by output contract: this pipeline only ever asks for the single mask of token 0, which holds IoU >= 0.9995 against
        the reference with every block GEMM at the 1x f16 rate (C2 fixtures): split 15; a multimask pipeline
        (InstancePipeline(multimask=True)) runs in the model's own default, which at ViT-H adds the v third of qkv + proj on
        hi + lo operands (split 79: what the three multimask tokens need for IoU >= 0.999, C4 fixtures; 0.90x the throughput).
        An explicit choice -- builder ``options={"split": ...}`` or SAMRS_SPLIT -- is never overridden.
        "engine" = the engine's option as it stands at each call; an int = that mode (and, for a multimask pipeline, the
        caller's consent to run its multimask predicts in it: option "allow_reduced").
        batch_decode: decode the prompts of every tile of a batch in one ``Engine.predict_multi`` call (one decoder chain per
        batch instead of one per tile and box chunk); painting, RLE and PNG encoding then run per tile as before, and every
        output is the same byte for byte.  True / False: on / off; a chain holds the engine's "decode_prompts" prompts (its
        max_prompts unless somebody raised it) and a longer batch is cut into chunks of that size again.  "auto" (default): on
        where a whole batch fits ONE chain and no tile is decoded in several chunks (``resolve_batch_decode``), raising the
        engine's "decode_prompts" to batch x max_boxes once, here, when it is smaller (13.5 MB of workspace per prompt); off
        otherwise, and off when the engine refuses the capacity.  ``batch_decode_on`` / ``batch_decode_reason`` say what it became.
        min_region_area: > 0 removes, on the device and before anything else reads the masks, every 8-connected island
        (region_mode "islands"), hole ("holes") or both ("both": holes first) of fewer than that many pixels
        (``Engine.clean_masks`` = segment_anything's ``remove_small_regions``): class map, areas, class statistics, RLE strings,
        device PNGs and kept masks all see the cleaned masks, and ``TileResult.changed`` counts the pixels changed per
        instance.  0 (default) issues no call at all.
        mask_boxes: derive, on the decode stream and from the masks that become the output (after the clean-up where that is
        on), each mask's tight hbox, its minimum-area rotated box and the record behind it (``Engine.mask_boxes``):
        ``TileResult.mask_hbox`` / ``mask_rbox`` / ``mask_record``.  False (default) launches and allocates nothing.
        quality: score every mask on the decode stream, before anything else reads it (``Engine.score_masks``, offset 1.0, the
        box in the original frame as it was staged): ``TileResult.score_counts`` (``quality.stability`` /
        ``quality.inside_fraction`` turn them into the two scores), ``TileResult.quality`` = the decoder's predicted IoU, and
        ``TileResult.kept``.  min_stability / min_pred_iou / min_inside_box: a threshold > 0 implies `quality` and drops the
        instances that fail it (``Engine.filter_masks``; the rule: ``quality.keep_rule``): a dropped mask is zeroed on the device
        before the clean-up, the mask boxes, the painting and the RLE encoding, so it paints nothing, has area 0, counts in no
        class statistic and ``kept`` is False for it.  Without a threshold every output but the three new fields is byte for byte
        what quality=False gives.  quality=False with no threshold (default) launches and allocates nothing new.
        polygons: trace, on the decode stream and from the masks as they go out (after the quality gate and the clean-up), each
        mask's outline as polygons on the pixel lattice -- outer rings and holes (``Engine.mask_polygons``):
        ``TileResult.polygons(j)`` / ``polygon_table`` / ``polygon_rings`` / ``polygon_vertices``.  A dropped or empty mask has no
        rings.  `polygon_buffer_mb`: the device buffer for one batch's vertices and ring records (two of them; 12 bytes per vertex
        with its share of ring records); a batch that overflows it raises, naming the option.  `polygon_max_edges`: a mask with
        more crack edges is not traced and yields None.  Every other output is byte for byte what polygons=False gives, and
        False (default) launches and allocates nothing.
        polygon_epsilon: > 0 (pixels; needs polygons=True) simplifies the batch's polygon stream once, on the decode stream, after
        the batch's last ``mask_polygons`` and before the download (``Engine.simplify_polygons``: Douglas-Peucker per ring at
        round(16 * polygon_epsilon) / 16 pixels, in integers): ``polygons(j)``, ``polygon_table``, ``polygon_rings`` and
        ``polygon_vertices`` then hold the simplified rings (a ring record's area stays the traced ring's), ``polygon_eps_q`` the
        tolerance in sixteenths.  Every other output is unchanged; 0.0 (default) makes no call and changes no byte.
        polygon_iou: (needs polygons=True) what the rings that are handed out cost against the mask they were traced from, counted
        while the mask is still on the device: after each ``mask_polygons`` call the rows it placed are simplified at once (instead
        of the whole batch at the end; the simplified rings depend on the ring and the tolerance only, so every polygon output is
        bit-equal to polygon_iou=False) and filled again (``Engine.fill_polygons`` without a mask output, `ref` = the chunk's
        masks): ``TileResult.polygon_counts`` [n_boxes, 3] = pixels of the fill (-1: not traced), of the mask, of both, and
        ``TileResult.polygon_iou(j)``.  With polygon_epsilon 0 every traced instance reports its area three times: a self-check
        of tracing and filling.  False (default) launches and allocates nothing and leaves the call sequence as it is.
        overlap: what becomes of a pixel at which several masks of a tile are set.  "order" (default): today's behaviour -- the
        masks stay as they are and the class map follows the painting order, a later box wins; nothing is launched or allocated.
        "logit" / "smallest": the pixel is given to exactly one instance on the device, in place (``Engine.resolve_overlaps``):
        the mask with the highest postprocessed logit there, or the mask with the fewest set pixels (equal areas fall to the
        logit); exact ties go to the later box, as painting does.  The stage runs after the quality gate and the clean-up and
        before the mask boxes, the polygons, the painting and the RLE encoding, so areas, class statistics, class map, PNGs, RLE
        strings, boxes, polygons and kept masks are all those of the disjoint masks, and the class map no longer depends on the
        box order except at exact ties; ``TileResult.removed`` counts the pixels taken from each instance.  All masks of a tile
        have to be on the device at once for this: a tile's boxes are decoded in ONE predict call whatever `box_batch` says (the
        engine cuts it into chains of its own), so n_boxes x H x W mask bytes live at once (512 MiB for 512 boxes of a 1024^2
        tile).  Under batch_decode the tile's rows of the batch's call are used as they are."""
        from .transforms import ResizeLongestSide
        refuse_boundary_option("TilePipeline", "Boundary AP needs the instance pipeline's ground truth", boundary=boundary)
        lut, poly_vertices = validate_output_options(min_region_area, region_mode, polygons, polygon_buffer_mb, polygon_max_edges, png_lut,
                                                     overlap, polygon_epsilon, polygon_iou)
        self.polygon_eps_q = polygon_eps_q(polygon_epsilon, bool(polygons))
        self.polygon_iou = bool(polygon_iou)
        vlut, self.vis_alpha = validate_vis_options(vis_lut, vis_alpha, vis_buffer_mb)
        self.vis = vlut is not None
        self.overlap = overlap
        self.min_region_area, self.region_mode = int(min_region_area), region_mode
        self.thresholds = (float(min_stability), float(min_pred_iou), float(min_inside_box))
        if any(t != t or t < 0 for t in self.thresholds):
            raise ValueError("min_stability, min_pred_iou and min_inside_box must be >= 0 (0 = off)")
        self.filter = any(t > 0 for t in self.thresholds)
        self.quality = bool(quality) or self.filter
        eng = sam.engine
        if eng is None:
            raise RuntimeError("move the model to the GPU first: sam.to('cuda')")
        self.split_mode = self._choose_split(sam, precision, multimask=_multimask)
        # consent to reduced-precision multimask predicts only means something for a pipeline that issues them
        self.allow_reduced = _multimask and isinstance(precision, int) and not isinstance(precision, bool)
        self.eng = eng
        if self.split_mode is not None:
            # fail HERE when the engine cannot run the mode (e.g. a block-GEMM bit whose lo weights were not finalized), not
            # mid-run inside _encode after _stage has queued H2D copies and recorded events (round-4 advisor finding)
            with self._mode():
                pass
        if out_depth < 2:
            raise ValueError("out_depth must be >= 2: batch k-1's results are still on loan to the sink when batch k decodes")
        if eng.max_images < 2 * batch:
            raise ValueError(f"TilePipeline(batch={batch}) needs an engine with max_images >= {2 * batch} "
                             f"(two embedding slot sets); got {eng.max_images}")
        self.sam, self.eng, self.dev = sam, eng, eng.device
        self.batch, self.box_batch, self.keep_masks, self.max_boxes = batch, box_batch, keep_masks, max_boxes
        self.rle = rle
        self.batch_decode, self.batch_decode_reason = self._resolve_batch_decode(batch_decode)
        self.batch_decode_on = self.batch_decode
        self.png = png_lut is not None
        self.side = sam.cfg.img_size
        self.transform = ResizeLongestSide(sam.image_encoder.img_size)
        self.class_pixels = torch.zeros(n_classes, dtype=torch.int64, device=self.dev)
        self.class_instances = torch.zeros(n_classes, dtype=torch.int64, device=self.dev)
        dev, side = self.dev, self.side
        # (round 5, measured: creating the encoder stream at the device's highest priority changes nothing -- 143.7 against 144.0
        # images/s over three alternations on one box; the streams stay at the default priority)
        self.s_h2d, self.s_enc, self.s_dec = (torch.cuda.Stream(dev) for _ in range(3))
        self.device_inputs = device_inputs
        self.pin_in = None
        if not device_inputs:
            self.pin_in = [torch.empty(batch, side, side, 3, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.mask_boxes, self.polygons = bool(mask_boxes), bool(polygons)
        self.dev_in = [torch.empty(batch, side, side, 3, dtype=torch.uint8, device=dev) for _ in range(2)]
        bw = self.BOX_WIDTH
        self.pin_box = [torch.empty(batch * max_boxes, bw, dtype=torch.float32).pin_memory() for _ in range(2)]
        self.pin_lab = [torch.empty(batch * max_boxes, dtype=torch.int32).pin_memory() for _ in range(2)]
        self.dev_box = [torch.empty(batch * max_boxes, bw, dtype=torch.float32, device=dev) for _ in range(2)]
        self.dev_lab = [torch.empty(batch * max_boxes, dtype=torch.int32, device=dev) for _ in range(2)]
        self.seg_dev = [torch.empty(batch, side, side, dtype=torch.uint8, device=dev) for _ in range(2)]
        # the fixed per-box outputs: one declaration each (output_tables), two device tables per entry under the entry's name
        self.tables = output_tables(self.min_region_area, self.mask_boxes, self.quality, self.gt, rle, self.INSTANCE, self.overlap,
                                    self.ap, self.boundary, self.polygon_iou)
        for t in self.tables:
            setattr(self, t.dev, [t.alloc(batch, max_boxes, dev) for _ in range(2)])
        # the packed outputs, per input set: the payload (16-byte aligned entries) here, cursor and table in the stream
        self.streams: List[PackedStream] = []
        if rle or self.png or polygons or self.vis:
            self.s_d2h = torch.cuda.Stream(dev)
        nbm = batch * max_boxes
        if rle:      # the batch's RLE strings; (offset, length, n_counts) per box
            self.rle_dev = [torch.empty(rle_buffer_mb << 20, dtype=torch.uint8, device=dev) for _ in range(2)]
            self.rle_out = PackedStream(self, "rle", nbm, (3,), [("rle_dev", (), torch.uint8, 1 << 20)],
                                        lambda tab, used: check_packed(tab, used[0], "batch", self.rle_dev[0].numel() >> 20))
            self.streams.append(self.rle_out)
            if self.gt:      # InstancePipeline(gt=True): the ground-truth masks' strings beside them
                self.gt_rle_dev = [torch.empty_like(t) for t in self.rle_dev]
                self.gt_rle_out = PackedStream(self, "gt_rle", nbm, (3,), [("gt_rle_dev", (), torch.uint8, 1 << 20)],
                                               lambda tab, used: check_packed(tab, used[0], "batch", self.gt_rle_dev[0].numel() >> 20))
                self.streams.append(self.gt_rle_out)
        if self.png:   # the LUT once; the batch's PNG files; (offset, length) of the gray and the colour file per tile
            self.png_lut = torch.from_numpy(lut).to(dev)
            self.png_buffer_mb = int(png_buffer_mb) if png_buffer_mb else 6 * batch
            self.png_dev = [torch.empty(self.png_buffer_mb << 20, dtype=torch.uint8, device=dev) for _ in range(2)]
            self.png_out = PackedStream(self, "png", batch, (2, 2), [("png_dev", (), torch.uint8, 1 << 20)],
                                        lambda tab, used: check_packed(tab, used[0], "batch", self.png_dev[0].numel() >> 20,
                                                                       what="PNG buffer too small: a file", knob="png_buffer_mb"))
            self.streams.append(self.png_out)
        if self.vis:   # the LUT once; one batch's blended pixels (used on s_dec alone); the batch's overlay files; (offset, length) per tile
            from .engine import png_rgb_bound
            self.vis_lut = torch.from_numpy(vlut).to(dev)
            self.vis_buffer_mb = int(vis_buffer_mb) if vis_buffer_mb else (batch * png_rgb_bound(side, side) >> 20) + 1
            self.vis_rgb = torch.empty(batch, side, side, 3, dtype=torch.uint8, device=dev)
            self.vis_dev = [torch.empty(self.vis_buffer_mb << 20, dtype=torch.uint8, device=dev) for _ in range(2)]
            self.vis_src: List[list] = [[], []]         # per input set: each tile's original pixels on the device
            self.vis_out = PackedStream(self, "vis", batch, (2,), [("vis_dev", (), torch.uint8, 1 << 20)],
                                        lambda tab, used: check_packed(tab, used[0], "batch", self.vis_dev[0].numel() >> 20,
                                                                       what="overlay buffer too small: a file", knob="vis_buffer_mb"))
            self.streams.append(self.vis_out)
        if self.polygons:   # the batch's vertices and ring records; the cursor counts both; five table columns per box
            self.polygon_buffer_mb, self.polygon_max_edges = int(polygon_buffer_mb), int(polygon_max_edges)
            self.poly_vert_dev = [torch.empty(poly_vertices, 2, dtype=torch.int32, device=dev) for _ in range(2)]
            self.poly_ring_dev = [torch.empty(poly_vertices // 4, 4, dtype=torch.int32, device=dev) for _ in range(2)]
            self.poly_out = PackedStream(self, "polygons", nbm, (5,), [("poly_vert_dev", (2,), torch.int32, 1 << 16),
                                                                        ("poly_ring_dev", (4,), torch.int32, 1 << 14)],
                                         lambda tab, used: check_polygons(tab, used[0], used[1], "batch", self.polygon_buffer_mb))
            self.streams.append(self.poly_out)
        self.ev_h2d = [torch.cuda.Event() for _ in range(2)]
        self.ev_enc = [torch.cuda.Event() for _ in range(2)]
        self.ev_dec = [torch.cuda.Event() for _ in range(2)]
        self.ev_in_free = [torch.cuda.Event() for _ in range(2)]     # encoder has consumed input set b
        self.free_out: "queue.Queue[_OutBuf]" = queue.Queue()
        for _ in range(out_depth):
            self.free_out.put(_OutBuf(batch, side, max_boxes, self.tables, self.streams))

    def _resolve_batch_decode(self, batch_decode) -> Tuple[bool, str]:
        """(on, why).  "auto": the pure rule, then the engine's own answer to the capacity it asks for."""
        from .engine import EngineError
        if batch_decode != "auto":
            return bool(batch_decode), "explicit"
        eng = self.eng
        try:
            capacity = eng.get_option("decode_prompts")
        except (AssertionError, EngineError):                    # a library without the option: chains of max_prompts
            capacity = eng.max_prompts
        on, want, why = resolve_batch_decode("auto", self.batch, self.box_batch, self.max_boxes, eng.max_prompts, eng.max_images, capacity)
        if on and want is not None:
            try:
                eng.set_option("decode_prompts", want)
            except (AssertionError, EngineError) as exc:         # refused (range, memory): the engine is as it was
                return False, f"the engine refused decode_prompts={want}: {exc}"
        return on, why

    @staticmethod
    def _choose_split(sam, precision, multimask: bool) -> Optional[int]:
        """The "split" mode a pipeline's own calls run in; None = whatever the engine's option says at each call."""
        from .engine import SPLIT_DEFAULT
        if precision == "engine":
            return None
        if precision == "auto":
            if "split" in getattr(sam, "options", {}) or "SAMRS_SPLIT" in os.environ:
                return None                                          # an explicit choice for the whole engine stands
            return int(getattr(sam, "default_split", SPLIT_DEFAULT)) if multimask else SPLIT_DEFAULT
        return int(precision)

    @contextlib.contextmanager
    def _mode(self):
        """The engine in this pipeline's operand-split mode for the calls inside the block (host-side state read at launch)."""
        if self.split_mode is None:
            yield
            return
        kw = {"split": self.split_mode}
        if self.allow_reduced:
            kw["allow_reduced"] = 1
        with self.eng.options(**kw):
            yield

    # -- stage A: stage tiles + boxes of one batch, H2D on s_h2d ------------------------------------------------
    def _stage(self, b: int, items: List[WorkItem]):
        tiles = []         # per image: (device tensor uint8 [h, w, 3] with long side == img_size, original (H, W))
        if self.vis:
            self.vis_src[b] = []
        same = True
        n_off = 0
        offs = []
        self.ev_in_free[b].synchronize()                  # pinned / device input set b is free again (host wait: the
        for i, it in enumerate(items):                    # pinned buffer must not be overwritten under an in-flight copy)
            nb = len(it.labels)
            if nb > self.max_boxes:
                raise ValueError(f"{nb} boxes on one image > max_boxes={self.max_boxes}")
            self.pin_box[b][n_off:n_off + nb] = torch.as_tensor(np.asarray(it.boxes, dtype=np.float32).reshape(-1, self.BOX_WIDTH))
            self.pin_lab[b][n_off:n_off + nb] = torch.as_tensor(np.asarray(it.labels).astype(np.int32))
            offs.append((n_off, nb))
            n_off += nb
        with torch.cuda.stream(self.s_h2d):
            self.s_h2d.wait_event(self.ev_dec[b])          # the decoder of batch k-2 read box / label set b
            self.dev_box[b][:n_off].copy_(self.pin_box[b][:n_off], non_blocking=True)
            self.dev_lab[b][:n_off].copy_(self.pin_lab[b][:n_off], non_blocking=True)
            for i, it in enumerate(items):
                img = it.image
                H, W = int(img.shape[0]), int(img.shape[1])
                native = (H == self.side and W == self.side)
                if isinstance(img, torch.Tensor) and img.is_cuda:
                    t = img
                    if native:
                        self.dev_in[b][i].copy_(t, non_blocking=True)
                        t = self.dev_in[b][i]
                elif native:
                    src = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
                    if src.is_pinned():                                           # caller-owned pinned memory: straight H2D
                        self.dev_in[b][i].copy_(src, non_blocking=True)
                    else:
                        if self.pin_in is None:                                   # device_inputs=True promised resident tiles
                            self.pin_in = [torch.empty(self.batch, self.side, self.side, 3, dtype=torch.uint8).pin_memory()
                                           for _ in range(2)]
                        # host memcpy into pinned staging: numpy's (one thread, lock released), not Tensor.copy_, which fans a
                        # 3 MiB copy out over every OpenMP thread -- 5.6 ms instead of 0.1 ms on a 16-CPU slice of a 256-thread host
                        np.copyto(self.pin_in[b][i].numpy(), src.numpy())
                        self.dev_in[b][i].copy_(self.pin_in[b][i], non_blocking=True)
                    t = self.dev_in[b][i]
                else:
                    src = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
                    t = src.to(self.dev)                                          # odd sizes: plain upload, then
                if self.vis:                                                      # the blend reads the image's own pixels on s_dec
                    orig = t.contiguous()
                    if not native:
                        orig.record_stream(self.s_dec)
                    self.vis_src[b].append(orig)
                if not native:
                    t = self.transform.apply_image_device(t.contiguous())         # PIL-exact resize on the GPU
                    t.record_stream(self.s_enc)                                   # allocated on s_h2d, read by the encoder
                    same = False
                tiles.append((t, (H, W)))
            self.ev_h2d[b].record(self.s_h2d)
        return tiles, same, offs

    def _encode(self, b: int, tiles, same: bool):
        n = len(tiles)
        with torch.cuda.stream(self.s_enc):
            self.s_enc.wait_event(self.ev_h2d[b])
            self.s_enc.wait_event(self.ev_dec[b])                  # decoder is done with embedding slot set b
            with self._mode():
                if same:
                    self.eng.set_images(self.dev_in[b][:n], b * self.batch)
                else:
                    self.eng.set_images_ragged([t for t, _ in tiles], b * self.batch)
            self.ev_enc[b].record(self.s_enc)
            if not self.vis:                                       # with vis_lut the blend reads input set b after the encoder: _decode
                self.ev_in_free[b].record(self.s_enc)

    multimask = False      # InstancePipeline sets these five
    gt = False
    ap = False
    boundary = False
    INSTANCE = False

    def _tile_prompts(self, b: int, tile, hw, off: int, nb: int):
        """(boxes, point_coords, point_labels, mask_input) of the nb staged annotations from row `off` of input set b: a tile's
        (batch_decode) or a chunk's.  The only place that turns annotations into prompts."""
        in_size = (int(tile.shape[0]), int(tile.shape[1]))
        return self._input_frame_boxes(self.dev_box[b][off:off + nb], hw, in_size), None, None, None           # :174

    def _decode_multi(self, b: int, tiles, offs):
        """batch_decode: the prompts of every tile of batch b in one predict_multi call -> per tile (masks, iou, low)."""
        per = [self._tile_prompts(b, t, hw, off, nb) for (t, hw), (off, nb) in zip(tiles, offs)]
        args = [None if per[0][j] is None else torch.cat([p[j] for p in per]) for j in range(4)]
        masks, iou, low = self.eng.predict_multi([b * self.batch + i for i in range(len(tiles))], [nb for _, nb in offs], *args,
                                               self.multimask, False, [(int(t.shape[0]), int(t.shape[1])) for t, _ in tiles],
                                               [tuple(hw) for _, hw in tiles])
        return list(zip(masks, iou, low))

    def _chunk_masks(self, b: int, i: int, tile, hw, off: int, s: int, e: int, pre):
        """(masks, iou, low) of prompts s..e of tile i: rows of `pre`, the tile's output of _decode_multi (batch_decode), or with
        pre None one predict call of its own."""
        if pre is not None:
            return pre[0][s:e], pre[1][s:e], pre[2][s:e]
        in_size = (int(tile.shape[0]), int(tile.shape[1]))
        return self.eng.predict(b * self.batch + i, *self._tile_prompts(b, tile, hw, off + s, e - s), self.multimask, False, in_size,
                                tuple(hw))

    def _decode_tile(self, b: int, i: int, tile, hw, off: int, nb: int, out: _OutBuf, pre=None) -> None:
        """Everything the reference does per image after set_image (main_sam_hbox_semantic.py:157-206), on s_dec.  pre: the
        tile's (masks, iou, low) from _decode_multi (batch_decode), or None to predict here, chunk by chunk."""
        eng, (H, W) = self.eng, hw
        in_size = (int(tile.shape[0]), int(tile.shape[1]))
        native = (H, W) == (self.side, self.side)
        seg = self.seg_dev[b][i] if native else torch.full((H, W), 255, dtype=torch.uint8, device=self.dev)
        kept = []
        resolve = self.overlap != "order"
        # :157-181; the overlap stage needs every mask of the tile at once: one chunk
        for s, e in ([(0, nb)] if nb else []) if resolve else box_chunks(nb, self.box_batch):
            masks, iou, low = self._chunk_masks(b, i, tile, hw, off, s, e, pre)
            if self.quality:                                                      # score, then filter: before anything reads the masks
                self._score(b, i, off, s, e, masks[:, 0], iou, low, in_size, (H, W))
            if self.min_region_area:                                              # before anything else reads the masks
                eng.clean_masks(masks[:, 0], self.min_region_area, self.region_mode, areas_out=False,     # paint counts them
                                changed_out=self.chg_dev[b][i, s:e])
            if resolve:                                                           # of the masks as gated and cleaned; "smallest": low breaks ties
                eng.resolve_overlaps(masks[:, 0], self.overlap, low=low, input_size=in_size, owner_out=False, before_out=False,
                                     removed_out=self.rem_dev[b][i, s:e])
            if self.mask_boxes:
                eng.mask_boxes(masks[:, 0], (0, 0), self.hbox_dev[b][i, s:e], self.rbox_dev[b][i, s:e], self.rec_dev[b][i, s:e])
            if self.polygons:                                                     # of the masks as they go out
                eng.mask_polygons(masks[:, 0], (0, 0), self.polygon_max_edges, self.poly_vert_dev[b], self.poly_ring_dev[b],
                                  self.poly_out.cur[b], self.poly_out.tab[b][off + s:off + e])
                if self.polygon_iou:                                              # while the chunk's masks are here: its rows, simplified now
                    rows = self.poly_out.tab[b][off + s:off + e]
                    if self.polygon_eps_q:
                        eng.simplify_polygons(rows, self.poly_ring_dev[b], self.poly_vert_dev[b], self.poly_out.cur[b],
                                              self.polygon_eps_q / 16.0)
                    eng.fill_polygons(rows, self.poly_ring_dev[b], self.poly_vert_dev[b], (H, W), (0, 0), out=False, ref=masks[:, 0],
                                      counts_out=self.pcnt_dev[b][i, s:e])
            eng.paint(masks[:, 0], self.dev_lab[b][off + s:off + e], seg, self.class_pixels, self.class_instances,
                      areas_out=self.area_dev[b][i, s:e])
            if self.rle:                                                          # :201-202, on the device
                eng.rle_encode(masks[:, 0], self.rle_dev[b], self.rle_out.cur[b], self.rle_out.tab[b][off + s:off + e])
            if self.keep_masks:
                kept.append(masks[:, 0].view(torch.uint8))
        if self.png and not native:                                              # an odd-sized tile: its own call
            eng.png_encode(seg, self.png_lut, self.png_dev[b], self.png_out.cur[b], self.png_out.tab[b][i:i + 1])
        if self.vis and not native:                                              # the same for its overlay, from the uploaded original
            over = eng.blend_labels(self.vis_src[b][i], seg, self.vis_lut, self.vis_alpha)
            eng.png_encode_rgb(over, self.vis_dev[b], self.vis_out.cur[b], self.vis_out.tab[b][i:i + 1])
        if native:
            out.seg[i].copy_(seg, non_blocking=True)
        else:
            out.odd[i] = seg.cpu()                    # other sizes (DIOR 800^2, HRSC): synchronous copy, rare path
        # keep_masks: the full-resolution masks themselves (n MiB per tile instead of 1 MiB, copied synchronously) -- a
        # debugging / evaluation mode; the reference's pkl contract needs only their RLE (rle=True, encoded on the device)
        out.masks[i] = torch.cat(kept).cpu() if (self.keep_masks and kept) else None

    STABILITY_OFFSET = 1.0     # the reference's stability_score_offset (automatic_mask_generator.py:43)

    def _score(self, b: int, i: int, off: int, s: int, e: int, masks, iou, low, in_size, hw) -> None:
        """quality: the counts of one chunk's masks from their low-resolution logits into the batch's table (the boxes as staged:
        original frame), the predicted IoU beside them, and with a threshold the gate, which zeroes the dropped masks in place."""
        eng = self.eng
        counts = eng.score_masks(low[:, 0], in_size, hw, self.STABILITY_OFFSET, boxes=self.dev_box[b][off + s:off + e],
                                 counts_out=self.cnt_dev[b][i, s:e])
        self.qual_dev[b][i, s:e].copy_(iou[:, 0])
        if self.filter:
            eng.filter_masks(masks, counts, self.qual_dev[b][i, s:e], *self.thresholds, keep_out=self.keep_dev[b][i, s:e])

    def _input_frame_boxes(self, boxes: torch.Tensor, hw, in_size) -> torch.Tensor:
        """apply_boxes_torch (utils/transforms.py:83-91).  When the tile already has the encoder's input size both scale
        factors are exactly 1.0 and x * 1.0f == x bit for bit, so the boxes are handed over as they are (no launches)."""
        if tuple(hw) == tuple(in_size):
            return boxes
        return self.transform.apply_boxes_torch(boxes, hw)

    def _decode(self, b: int, items, tiles, offs, out: _OutBuf):
        with torch.cuda.stream(self.s_dec):
            self.s_dec.wait_event(self.ev_enc[b])
            self.seg_dev[b].fill_(255)                                               # main_sam_hbox_semantic.py:162
            for st in self.streams:
                st.reset(b)
            with self._mode():
                pre = self._decode_multi(b, tiles, offs) if self.batch_decode and sum(nb for _, nb in offs) else None
                for i, ((t, hw), (off, nb)) in enumerate(zip(tiles, offs)):
                    self._decode_tile(b, i, t, hw, off, nb, out, None if pre is None else pre[i])
            n_rows = sum(nb for _, nb in offs)
            if self.polygons and self.polygon_eps_q and n_rows and not self.polygon_iou:   # the batch's rings, once: its rows are 0 .. n_rows - 1
                self.eng.simplify_polygons(self.poly_out.tab[b][:n_rows], self.poly_ring_dev[b], self.poly_vert_dev[b],
                                           self.poly_out.cur[b], self.polygon_eps_q / 16.0)
            if self.png:
                self._encode_png(b, tiles)
            if self.vis:
                self._encode_vis(b, tiles)
            for t in self.tables:
                out.tables[t.field].copy_(getattr(self, t.dev)[b], non_blocking=True)
            for st in self.streams:
                st.copy_table(b, out)
            self.ev_dec[b].record(self.s_dec)
            out.done.record(self.s_dec)

    def _native_runs(self, tiles) -> List[Tuple[int, int]]:
        """[i0, i1) of every run of consecutive native (side x side) tiles of a batch."""
        native = [i for i, (_, hw) in enumerate(tiles) if tuple(hw) == (self.side, self.side)]
        runs: List[List[int]] = []
        for i in native:
            if runs and runs[-1][-1] == i - 1:
                runs[-1].append(i)
            else:
                runs.append([i])
        return [(r[0], r[-1] + 1) for r in runs]

    def _encode_vis(self, b: int, tiles) -> None:
        """The overlays of the batch's native tiles, on s_dec after painting: per run of consecutive native tiles one blend of input
        set b's pixels with the painted class maps and one samrs_png_encode_rgb call.  Odd-sized tiles were done in _decode_tile.
        Every blend of the batch is enqueued once this returns: input set b goes back to staging."""
        runs = self._native_runs(tiles)
        for i0, i1 in runs:
            self.eng.blend_labels(self.dev_in[b][i0:i1], self.seg_dev[b][i0:i1], self.vis_lut, self.vis_alpha, out=self.vis_rgb[i0:i1])
        self.ev_in_free[b].record(self.s_dec)
        for i0, i1 in runs:
            self.eng.png_encode_rgb(self.vis_rgb[i0:i1], self.vis_dev[b], self.vis_out.cur[b], self.vis_out.tab[b][i0:i1])

    def _encode_png(self, b: int, tiles) -> None:
        """gray + colour PNG of the batch's native tiles: one samrs_png_encode_labels call per run of consecutive native tiles
        (one call for a batch of native tiles), on s_dec after painting.  Odd-sized tiles were encoded in _decode_tile."""
        for i0, i1 in self._native_runs(tiles):
            self.eng.png_encode(self.seg_dev[b][i0:i1], self.png_lut, self.png_dev[b], self.png_out.cur[b], self.png_out.tab[b][i0:i1])

    def _finish(self, pending, sink):
        items, offs, out, b = pending
        out.done.synchronize()
        odd = out.odd
        res = []
        n_boxes = sum(nb for _, nb in offs)
        if self.rle:
            rtab, (rdat,), _ = self.rle_out.fetch(b, out, n_boxes)
            if self.gt:
                ttab, (tdat,), _ = self.gt_rle_out.fetch(b, out, n_boxes)
        if self.png:                                        # two table rows per tile: its gray and its colour file
            ptab, (pdat,), _ = self.png_out.fetch(b, out, 2 * len(items))
            ptab = ptab.reshape(-1, 2, 2)
        if self.vis:
            vtab, (vdat,), _ = self.vis_out.fetch(b, out, len(items))
        if self.polygons:
            gtab, (gvert, gring), (nv, nr) = self.poly_out.fetch(b, out, n_boxes)
            gtab, gvert, gring = gtab.copy(), gvert[:nv].numpy(), gring[:nr].numpy()
        for i, (it, (off, nb)) in enumerate(zip(items, offs)):
            seg = (odd[i].numpy() if odd[i] is not None else None) if i in odd else out.seg[i].numpy()
            m = out.masks[i].numpy() if out.masks[i] is not None else None
            r = TileResult(it.key, seg, boxes=np.asarray(it.boxes), labels=np.asarray(it.labels), masks=m,
                           **{t.field: t.rows(out.tables[t.field][i] if t.per_tile else out.tables[t.field][i, :nb])
                              for t in self.tables})
            if seg is not None:
                r.size = (int(seg.shape[0]), int(seg.shape[1]))
            else:
                r.size = (int(it.image.shape[0]), int(it.image.shape[1]))
            if self.rle:
                r.rle_table, r.rle_data = rtab[off:off + nb], rdat.numpy()
                if self.gt:
                    r.gt_rle_table, r.gt_rle_data = ttab[off:off + nb], tdat.numpy()
            if self.png:
                r.png_table, r.png_data = ptab[i], pdat.numpy()
            if self.vis:
                r.vis_table, r.vis_data = vtab[i], vdat.numpy()
            if self.polygons:
                r.polygon_table, r.polygon_rings, r.polygon_vertices = gtab[off:off + nb], gring, gvert
            res.append(r)
        out.odd = {}
        release = lambda o=out: self.free_out.put(o)
        sink(res, release)

    @torch.no_grad()
    def run(self, batches: Iterable[List[WorkItem]], sink: Callable[[List[TileResult], Callable[[], None]], None]) -> int:
        """Drives `batches` (lists of <= batch WorkItems) through the pipeline.  `sink(results, release)` is called on the
        calling thread, in order, once a batch's class maps and areas are on the host; the arrays are views of a pinned
        ring buffer, so the sink (or whatever it hands them to) must call `release()` when it is done with them.
        Returns the number of tiles processed."""
        cur = torch.cuda.current_stream(self.dev)
        for st in (self.s_h2d, self.s_enc, self.s_dec):
            st.wait_stream(cur)
        n_tiles = 0
        staged = None        # batch k+1: staged, not yet encoded
        encoded = None       # batch k  : encoder issued
        decoding = None      # batch k-1: decoder issued, results not yet handed over
        it = iter(batches)
        k = 0
        while True:
            nxt = next(it, None)
            if nxt is not None:
                if len(nxt) < 1 or len(nxt) > self.batch:
                    raise ValueError(f"a batch must hold 1..{self.batch} work items")
                b = k & 1
                tiles, same, offs = self._stage(b, nxt)
                self._encode(b, tiles, same)
                staged = (b, nxt, tiles, offs)
                n_tiles += len(nxt)
                k += 1
            if encoded is not None:
                b, items, tiles, offs = encoded
                out = self.free_out.get()                              # blocks while the writers hold every buffer
                self._decode(b, items, tiles, offs, out)
                if decoding is not None:
                    self._finish(decoding, sink)
                decoding = (items, offs, out, b)
            encoded, staged = staged, None
            if nxt is None and encoded is None:
                break
        if decoding is not None:
            self._finish(decoding, sink)
        for st in (self.s_h2d, self.s_enc, self.s_dec):
            cur.wait_stream(st)
        return n_tiles


def batched(items: Iterable[WorkItem], batch: int) -> Iterator[List[WorkItem]]:
    buf: List[WorkItem] = []
    for it in items:
        buf.append(it)
        if len(buf) == batch:
            yield buf
            buf = []
    if buf:
        yield buf


class InstancePipeline(TilePipeline):
    """The instance drivers' recipe (main_sam_rhbox_mask_instance.py:125-168 / main_sam_rbox_mask_instance.py:125-164)
    on the same three-stream pipeline.  ``multimask=True`` is BASELINE.json configs[3]; the reference's own instance scripts all pass
    ``multimask_output=False`` (main_sam_rhbox_mask_instance.py:168, main_sam_rbox_mask_instance.py:164,
    main_sam_hbox_mask_instance.py:165): ``multimask=False`` is their configuration.  Annotations are
    rotated boxes [n, 4, 2]; ``prompt="box"`` feeds the enclosing hbox (min / max of the corners, :125-130) through
    ``apply_boxes_torch``, ``prompt="rbox_mask"`` rasterises the rbox into a +-1000 mask prompt on the GPU
    (``transforms.rbox_mask_prompts``).  Of the three masks per object the one with the highest predicted IoU is kept
    (SAM's own selection rule, `samrs_select_best` on the device); per object the host receives its area and quality (and with
    ``rle=True`` its COCO RLE), the kept masks stay in HBM (``last_masks``) unless keep_masks.  No class map is painted:
    ``TileResult.seg_mask`` is None and the class statistics stay zero (the instance drivers write neither).

    ``gt=True`` adds the evaluation of main_sam_rhbox_mask_instance.py:204-244 on the device: every ``WorkItem`` carries
    ``gt=(label_rgb, colors)``; the label image is staged with the tile, and after the best-mask selection `samrs_gt_match`
    counts per object |mask AND ground truth| and |ground truth| into ``TileResult.inter`` / ``gt_area`` (union = areas +
    gt_area - inter); with ``rle=True`` the ground-truth masks are RLE-encoded on the device too (``TileResult.gt_rle``)."""

    BOX_WIDTH = 8          # four (x, y) corners
    INSTANCE = True

    def __init__(self, sam, n_classes: int, prompt: str = "box", multimask: bool = True, fill_rule: str = "auto", gt: bool = False,
                 ap: bool = False, boundary: bool = False, dilation_ratio: float = 0.02, **kw):
        """prompt: "box" / "rbox_mask" (annotations = rotated boxes [n, 4, 2]) or "point"
        (main_sam_hbox_mask_instance.py:160-165: annotations = one foreground point [n, 2] per object, handed to the prompt
        encoder AS IS -- the reference does not run them through apply_coords -- labels all 1, no box, no mask;
        that driver uses multimask_output=False: pass multimask=False).
        ap (needs gt=True): COCO mask AP's per-image matching on the device, every prediction of a tile against every ground truth
        of it.  Each decode chunk packs its kept masks, as they go out, and its ground truth (straight from the staged label image)
        into bit planes -- an eighth of the mask bytes, kept for the whole tile while the masks come and go `box_batch` at a time;
        after the tile's last chunk ``Engine.mask_pair_counts`` and ``Engine.coco_match`` (score = the kept mask's predicted IoU)
        run on the decode stream and ``TileResult.ap_tables`` holds the fixed-size tables ``coco_ap.accumulate`` takes.  The plane
        buffers hold one tile and grow on demand (max_boxes x ceil(H W / 64) words each); tiles follow each other on one stream.
        False (default) launches and allocates nothing, and every other output is byte for byte the same either way.
        boundary (needs ap=True): Boundary AP's matching beside it (the rules: samrs_mask_boundary_bits in include/samrs_hip.h).  Two
        more plane buffers of the same size; after the tile's last chunk, on the decode stream, both stacks of planes are banded
        (``Engine.mask_boundary_bits``, d = ``coco_ap.boundary_dilation(H, W, dilation_ratio)``), counted a second time and matched by
        min(mask IoU, boundary IoU) into a second set of fixed-size tables: ``TileResult.boundary_tables``, which also holds the
        per-object band counts ``band_inter`` / ``band_area_d`` / ``band_area_g`` for the Boundary mIoU.  False (default) launches
        and allocates nothing, and every other output, ``ap_tables`` included, is byte for byte the same either way."""
        if prompt not in ("box", "rbox_mask", "point"):
            raise ValueError("prompt must be 'box', 'rbox_mask' or 'point'")
        if ap and not gt:
            raise ValueError("InstancePipeline(ap=True) matches predictions against the ground truth: it needs gt=True")
        if boundary and not ap:
            raise ValueError("InstancePipeline(boundary=True) is a second matching beside the mask AP's: it needs ap=True")
        if boundary and not (float(dilation_ratio) > 0):
            raise ValueError(f"dilation_ratio must be > 0, got {dilation_ratio!r}")
        self.ap = bool(ap)             # read by TilePipeline.__init__ (output_tables)
        self.boundary, self.dilation_ratio = bool(boundary), float(dilation_ratio)
        refuse_quality_options("InstancePipeline", "scoring the best-of-3 path is not built", **kw)
        refuse_overlap_option("InstancePipeline", "resolving the best-of-3 masks is not built", **kw)
        refuse_vis_option("InstancePipeline", "it paints no class map to blend", **kw)
        if prompt == "point":
            self.BOX_WIDTH = 2
        from . import transforms
        self.fill_rule = transforms.resolve_fill_rule(fill_rule)       # prompt="rbox_mask": the cv2.fillPoly span rule to reproduce
        if kw.get("png_lut") is not None:
            raise ValueError("InstancePipeline paints no class map: png_lut is a TilePipeline option")
        if kw.get("polygons"):
            raise ValueError("InstancePipeline does not trace polygons: polygons is a TilePipeline / ScenePipeline option")
        if kw.get("polygon_epsilon"):
            raise ValueError("InstancePipeline does not trace polygons: polygon_epsilon is a TilePipeline / ScenePipeline option")
        refuse_polygon_iou_option("InstancePipeline", "it traces no polygons", polygon_iou=kw.get("polygon_iou"))
        self.gt = bool(gt)             # read by TilePipeline.__init__: the ground-truth tables and stream are allocated with the rest
        super().__init__(sam, n_classes, precision=kw.pop("precision", "auto"), _multimask=bool(multimask), **kw)
        self.prompt, self.multimask = prompt, bool(multimask)
        self.last_masks = None
        if self.gt:
            dev, B, M = self.dev, self.batch, self.max_boxes
            self.pin_col = [torch.empty(B * M, 3, dtype=torch.uint8).pin_memory() for _ in range(2)]
            self.dev_col = [torch.empty(B * M, 3, dtype=torch.uint8, device=dev) for _ in range(2)]
            self.gt_lab: List[List[torch.Tensor]] = [[], []]          # per input set: the label images on the device
            self.ev_gt = [torch.cuda.Event() for _ in range(2)]
        if self.ap:                    # one tile's planes and pair counts, all used on s_dec alone
            M = self.max_boxes
            self.ap_words = 0
            self.ap_pred = self.ap_gt = None
            self.ap_inter = torch.empty(M * M, dtype=torch.int64, device=self.dev)
            self.ap_area = torch.empty(2, M, dtype=torch.int64, device=self.dev)
        if self.boundary:              # the bands of those planes and their pair counts, on s_dec too
            self.bd_pred = self.bd_gt = None
            self.bd_inter = torch.empty(self.max_boxes * self.max_boxes, dtype=torch.int64, device=self.dev)

    def _ap_planes(self, hw):
        """The tile's plane buffers [max_boxes, words] (prediction, ground truth), grown to the tile's size on the decode stream."""
        words = (int(hw[0]) * int(hw[1]) + 63) // 64
        if words > self.ap_words:
            self.ap_pred = self.ap_gt = None              # stream-ordered: the allocator hands the blocks out on s_dec again
            self.ap_pred = torch.empty(self.max_boxes * words, dtype=torch.int64, device=self.dev)
            self.ap_gt = torch.empty(self.max_boxes * words, dtype=torch.int64, device=self.dev)
            if self.boundary:
                self.bd_pred = self.bd_gt = None
                self.bd_pred = torch.empty(self.max_boxes * words, dtype=torch.int64, device=self.dev)
                self.bd_gt = torch.empty(self.max_boxes * words, dtype=torch.int64, device=self.dev)
            self.ap_words = words
        n = self.max_boxes * words
        return self.ap_pred[:n].view(self.max_boxes, words), self.ap_gt[:n].view(self.max_boxes, words)

    def _ap_match(self, b: int, i: int, nb: int, planes, hw=None) -> None:
        """After a tile's last chunk: its nb predictions against its nb ground truths, matched into the batch's tables; with
        `boundary` the bands of both stacks too, matched by the smaller IoU into the second set."""
        eng = self.eng
        pp, gp = (planes[0][:nb], planes[1][:nb]) if planes is not None else (torch.zeros(0, 1, dtype=torch.int64, device=self.dev),) * 2
        inter, ad, ag = eng.mask_pair_counts(pp, gp, self.ap_inter[:nb * nb].view(nb, nb), self.ap_area[0, :nb], self.ap_area[1, :nb])
        eng.coco_match(inter, ad, ag, self.qual_dev[b][i, :nb], max_det=AP_SHAPE[2], order_out=self.ap_order_dev[b][i],
                       match_out=self.ap_match_dev[b][i], dt_ignore_out=self.ap_ign_dev[b][i], n_valid_out=self.ap_nvalid_dev[b][i],
                       n_kept_out=self.ap_nkept_dev[b][i])
        if not self.boundary:
            return
        bp, bg = pp, gp
        if planes is not None:
            from .coco_ap import boundary_dilation
            d, words = boundary_dilation(hw[0], hw[1], self.dilation_ratio), pp.shape[1]
            bp = eng.mask_boundary_bits(pp, hw[0], hw[1], d, self.bd_pred[:nb * words].view(nb, words))
            bg = eng.mask_boundary_bits(gp, hw[0], hw[1], d, self.bd_gt[:nb * words].view(nb, words))
        band = eng.mask_pair_counts(bp, bg, self.bd_inter[:nb * nb].view(nb, nb), self.band_ad_dev[b][i, :nb], self.band_ag_dev[b][i, :nb])
        self.band_inter_dev[b][i, :nb].copy_(band[0].diagonal())
        eng.coco_match(inter, ad, ag, self.qual_dev[b][i, :nb], max_det=AP_SHAPE[2], order_out=self.bd_order_dev[b][i],
                       match_out=self.bd_match_dev[b][i], dt_ignore_out=self.bd_ign_dev[b][i], n_valid_out=self.bd_nvalid_dev[b][i],
                       n_kept_out=self.bd_nkept_dev[b][i], boundary=band)

    def _stage(self, b: int, items: List[WorkItem]):
        if not self.gt:
            return super()._stage(b, items)
        gts = []
        for it in items:                                  # check everything before anything is queued
            if it.gt is None:
                raise ValueError(f"InstancePipeline(gt=True): work item {it.key!r} carries no gt=(label_rgb, colors)")
            lab, col = np.asarray(it.gt[0]), np.asarray(it.gt[1])
            H, W = int(it.image.shape[0]), int(it.image.shape[1])
            if lab.dtype != np.uint8 or lab.shape != (H, W, 3):
                raise ValueError(f"work item {it.key!r}: label image {lab.dtype} {tuple(lab.shape)} does not match the image "
                                 f"(uint8 [{H}, {W}, 3])")
            if col.dtype != np.uint8 or col.shape != (len(it.labels), 3):
                raise ValueError(f"work item {it.key!r}: colors must be uint8 [{len(it.labels)}, 3], got {col.dtype} {tuple(col.shape)}")
            gts.append((lab, col))
        out = super()._stage(b, items)
        self.ev_gt[b].synchronize()                       # the last copies out of pin_col[b] have finished
        n_off, labs = 0, []
        for lab, col in gts:
            self.pin_col[b][n_off:n_off + len(col)] = torch.from_numpy(np.ascontiguousarray(col))
            n_off += len(col)
        with torch.cuda.stream(self.s_h2d):               # behind the wait for the decoder of batch k-2 (super()._stage)
            self.dev_col[b][:n_off].copy_(self.pin_col[b][:n_off], non_blocking=True)
            for lab, _ in gts:
                # through pinned memory, asynchronously: a pageable copy would hold this thread until the decoder of batch k-2
                # is done (the wait above), and the decoder would idle before batch k-1 is issued.  np.copyto, not copy_ (_stage)
                pin = torch.empty(lab.shape, dtype=torch.uint8, pin_memory=True)
                np.copyto(pin.numpy(), lab)
                t = pin.to(self.dev, non_blocking=True)   # the caching host allocator keeps `pin` until the copy is done
                t.record_stream(self.s_dec)                # allocated on s_h2d, read by the decoder
                labs.append(t)
            self.ev_gt[b].record(self.s_h2d)
        self.gt_lab[b] = labs
        return out

    def _tile_prompts(self, b: int, tile, hw, off: int, nb: int):
        from . import transforms
        in_size = (int(tile.shape[0]), int(tile.shape[1]))
        ann = self.dev_box[b][off:off + nb]
        if self.prompt == "box":
            polys = ann.view(-1, 4, 2)
            hb = torch.cat([polys.amin(1), polys.amax(1)], dim=1)                                   # :125-130
            return self._input_frame_boxes(hb, hw, in_size), None, None, None
        if self.prompt == "rbox_mask":
            side = 4 * self.sam.cfg.grid
            pr = (transforms.rbox_mask_prompts_device(ann.view(-1, 4, 2), hw, self.side, device=self.dev, fill_rule=self.fill_rule)
                  if nb else torch.empty(0, side, side, dtype=torch.float32, device=self.dev))
            return None, None, None, pr[:, None]
        return None, ann.view(-1, 1, 2), torch.ones(nb, 1, dtype=torch.int32, device=self.dev), None

    def _decode_tile(self, b, i, tile, hw, off, nb, out, pre=None) -> None:
        eng = self.eng
        kept = []
        if self.gt:
            self.s_dec.wait_event(self.ev_gt[b])
        planes = self._ap_planes(hw) if (self.ap and nb) else None
        for s, e in box_chunks(nb, self.box_batch):
            m, q, _ = self._chunk_masks(b, i, tile, hw, off, s, e, pre)
            # best of the C masks by predicted IoU, its quality and area: one pass on the device, straight into the tables
            mk, _, _ = eng.select_best(m, q, None, self.qual_dev[b][i, s:e], self.area_dev[b][i, s:e])
            if self.min_region_area:                      # the area table then holds the cleaned areas (select_best's are stale)
                eng.clean_masks(mk, self.min_region_area, self.region_mode, areas_out=self.area_dev[b][i, s:e],
                                changed_out=self.chg_dev[b][i, s:e])
            if self.mask_boxes:                           # of the kept mask, as it goes out
                eng.mask_boxes(mk, (0, 0), self.hbox_dev[b][i, s:e], self.rbox_dev[b][i, s:e], self.rec_dev[b][i, s:e])
            if self.rle:
                eng.rle_encode(mk, self.rle_dev[b], self.rle_out.cur[b], self.rle_out.tab[b][off + s:off + e])
            if self.gt:                                   # main_sam_rhbox_mask_instance.py:204-238, on the device
                gm = torch.empty_like(mk) if self.rle else None
                eng.gt_match(mk, self.gt_lab[b][i], self.dev_col[b][off + s:off + e], self.inter_dev[b][i, s:e],
                             self.gta_dev[b][i, s:e], gm)
                if self.rle:                              # instance_to_json.py:44-45
                    eng.rle_encode(gm, self.gt_rle_dev[b], self.gt_rle_out.cur[b], self.gt_rle_out.tab[b][off + s:off + e])
                    if self.mask_boxes:                   # the ground-truth masks are on the device here: their hbox too
                        eng.mask_boxes(gm, (0, 0), self.gt_hbox_dev[b][i, s:e], False, False)
            if planes is not None:                        # the chunk's planes stay while its masks go
                eng.pack_mask_bits(mk, planes[0][s:e])
                eng.pack_label_bits(self.gt_lab[b][i], self.dev_col[b][off + s:off + e], planes[1][s:e])
            kept.append(mk)
        if self.ap:
            self._ap_match(b, i, nb, planes, hw)
        self.last_masks = kept[-1].view(torch.bool) if kept else None
        out.masks[i] = torch.cat(kept).cpu() if (self.keep_masks and kept) else None
        out.odd[i] = None                      # instance pipelines paint no class map
