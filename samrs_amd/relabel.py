"""Rebuild every mask-only output from ``ins/*.pkl`` on the GPU, without an encoder pass.

    python -m samrs_amd.relabel --ins DIR --out OUT [--classes / --n-classes / --palette]
        [--min-region-area N --region-mode M] [--overlap order|smallest] [--mask-boxes] [--dota-txt]
        [--polygons [--polygon-max-edges E] [--polygon-epsilon E] [--polygon-iou]] [--masks-from rle|polygons] [--png-device]
        [--resume] [--box-batch B]

``DIR`` is a directory of ``*.pkl`` or a ``samrs_amd.generate`` output directory (its ``ins/`` is read): ours, a ``--resume``d run's,
or the published SAMRS pickles, which have the same keys.  The pickle is the durable record -- COCO RLE per instance, label, box,
size -- and everything ``generate`` decides after the decoder is a function of those masks alone.  Per pickle, in the order of
``driver.TilePipeline._decode_tile``: the entries' ``"mask"`` strings are decoded on the device (samrs_rle_decode) in chunks of
``--box-batch``, then ``clean_masks``, ``resolve_overlaps`` ("smallest", without logits; the whole image in one chunk),
``mask_boxes``, ``mask_polygons``, ``paint`` in list order (a later entry wins) into a 255-initialised map, ``rle_encode``, and the
gray / colour PNGs (host writers, or ``png_encode`` with --png-device).  Every key of an input entry survives; ``"mask"`` and
``"size"`` are replaced by those of the masks as they go out and the option keys are added under generate's names.  What needs the
decoder's logits or the image (--overlap logit, --quality and its thresholds, --vis) is refused.  Single process.
"""
from __future__ import annotations

import argparse
import json
import os
import pickle
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import generate, rle, tile_io
from .driver import (PolygonIoUStat, box_chunks, check_packed, check_polygons, polygon_eps_q, reduce_polygon_iou,
                     validate_output_options)
from .engine import RLE_STATUS
from .polygons import iou_from_counts, pack_rings, rings_of

NEEDS_LOGITS = "needs the decoder's logits, which ins/*.pkl does not hold"
NEEDS_IMAGE = "needs the image, which ins/*.pkl does not hold"
MASK_SOURCES = ("rle", "polygons")      # --masks-from: what every entry's mask is rebuilt from


def ins_dir_of(path: str) -> str:
    """`path` itself when it holds ``*.pkl``, else its ``ins/`` (a generate output directory)."""
    sub = os.path.join(path, "ins")
    if os.path.isdir(path) and not any(f.endswith(".pkl") for f in os.listdir(path)) and os.path.isdir(sub):
        return sub
    return path


def same_dir(a: str, b: str) -> bool:
    return os.path.realpath(a) == os.path.realpath(b)


def refusal(ns) -> Optional[str]:
    """Why these options cannot be served from the pickles alone, or None."""
    if ns.overlap == "logit":
        return f"--overlap logit {NEEDS_LOGITS}; use --overlap smallest (without logits equal areas go to the later entry)"
    for flag, on in (("--quality", ns.quality), ("--min-stability", ns.min_stability > 0), ("--min-pred-iou", ns.min_pred_iou > 0),
                     ("--min-inside-box", ns.min_inside_box > 0)):
        if on:
            return f"{flag} {NEEDS_LOGITS}"
    if ns.vis:
        return f"--vis {NEEDS_IMAGE}"
    if getattr(ns, "polygon_iou", False) and not (ns.polygons or ns.polygon_epsilon > 0):
        return "--polygon-iou scores the traced polygons against their masks: it needs --polygons or --polygon-epsilon"
    if same_dir(os.path.join(ns.out, "ins"), ins_dir_of(ns.ins)):
        return f"--out {ns.out}: its ins/ is the input directory, and the pickles being read would be overwritten; name another --out"
    return None


class _Parser(argparse.ArgumentParser):
    def parse_args(self, args=None, namespace=None):
        ns = super().parse_args(args, namespace)
        if ns.dota_txt:
            ns.mask_boxes = True
        why = refusal(ns)
        if why:
            self.error(why)
        if ns.box_batch < 1:
            self.error("--box-batch must be >= 1")
        return ns


def build_parser() -> argparse.ArgumentParser:
    ap = _Parser(description="ins/*.pkl -> class maps, statistics and per-instance outputs, re-derived on the GPU (no encoder pass)")
    ap.add_argument("--ins", required=True, help="a directory of *.pkl, or a generate output directory (its ins/ is read)")
    ap.add_argument("--out", required=True)
    ap.add_argument("--model", default="vit_tiny", help="the engine that hosts the kernels (no weights are used)")
    ap.add_argument("--classes", default=None, help="text file, one class name per line")
    ap.add_argument("--n-classes", type=int, default=18)
    ap.add_argument("--palette", default=None, help=".npy uint8 [n_classes, 3]")
    ap.add_argument("--box-batch", type=int, default=64, help="masks decoded and processed per chunk (--overlap smallest: the whole image)")
    ap.add_argument("--rle-buffer-mb", type=int, default=256, help="device buffer for one image's RLE strings")
    ap.add_argument("--resume", action="store_true", help="skip pickles whose gray / color / ins outputs already exist in --out")
    ap.add_argument("--png-level", type=int, default=tile_io.LEVEL_LABELS, help="as samrs_amd.generate")
    ap.add_argument("--png-device", action="store_true", help="encode gray/*.png and color/*.png on the GPU (byte-identical)")
    generate.add_region_arguments(ap, " Under --resume the totals cover the images processed in this run only.")
    generate.add_mask_box_arguments(ap, "every ins/<stem>.pkl entry gains \"mask_bbox\" (COCO [x, y, w, h]) and \"mask_rbox\" (float32 [4, 2]), "
                                        "None for an empty mask")
    ap.add_argument("--dota-txt", action="store_true", help="also write rbox/<stem>.txt as samrs_amd.generate does; implies --mask-boxes")
    ap.add_argument("--overlap", default="order", choices=["order", "logit", "smallest"],
                    help="order (default): the masks stay as they are, a later entry wins in the class map.  smallest: a pixel several "
                         "masks are set at goes to the mask with the fewest pixels (equal areas: the later entry); the entries gain "
                         "\"removed\".  logit is refused: " + NEEDS_LOGITS)
    ap.add_argument("--polygons", action="store_true", help="trace each mask's outline to polygons on the GPU, as samrs_amd.generate does")
    ap.add_argument("--polygon-buffer-mb", type=int, default=64, metavar="N")
    ap.add_argument("--polygon-max-edges", type=int, default=65536, metavar="E")
    ap.add_argument("--polygon-epsilon", type=float, default=0.0, metavar="E",
                    help="simplify the traced rings on the GPU at a tolerance of E pixels, as samrs_amd.generate does; implies --polygons")
    ap.add_argument("--polygon-iou", action="store_true",
                    help="fill the rings that are written again on the GPU and count them against their mask, as samrs_amd.generate does: "
                         "the entries gain 'polygon_iou', and OUT/statistic/polygon_iou.json is written; needs --polygons / --polygon-epsilon")
    ap.add_argument("--masks-from", default="rle", choices=list(MASK_SOURCES),
                    help="rle (default): every mask is decoded from its entry's \"mask\" RLE.  polygons: every mask is the even-odd fill, on "
                         "the GPU, of its entry's 'polygons' (at the pixel centres; holes follow from the rule, 'polygon_holes' is not "
                         "needed) -- a vector edit or a simplified outline becomes the class map, the statistics and the RLE again; an "
                         "entry whose 'polygons' is None falls back to its \"mask\", one with neither is an error")
    # named so that they are refused with a reason instead of "unrecognized arguments"
    ap.add_argument("--quality", action="store_true", help="refused: " + NEEDS_LOGITS)
    ap.add_argument("--min-stability", type=float, default=0.0, help="refused: " + NEEDS_LOGITS)
    ap.add_argument("--min-pred-iou", type=float, default=0.0, help="refused: " + NEEDS_LOGITS)
    ap.add_argument("--min-inside-box", type=float, default=0.0, help="refused: " + NEEDS_LOGITS)
    ap.add_argument("--vis", action="store_true", help="refused: " + NEEDS_IMAGE)
    return ap


def has_rle(e) -> bool:
    return isinstance(e, dict) and isinstance(e.get("mask"), dict) and "counts" in e["mask"] and "size" in e["mask"]


def load_entries(path: str, n_classes: int, masks_from: str = "rle") -> Tuple[List[dict], Optional[Tuple[int, int]]]:
    """(the entries of one pickle, their common mask size or None when no entry says it); ValueError, naming the file, for an entry
    without ``"mask"`` (`masks_from` "polygons": with neither ``"polygons"`` nor ``"mask"``), mixed sizes or a label outside
    0..n_classes-1."""
    with open(path, "rb") as f:
        entries = list(pickle.load(f))
    sizes = set()
    stem = os.path.basename(path)[:-4] if path.endswith(".pkl") else os.path.basename(path)
    for j, e in enumerate(entries):
        if masks_from == "polygons" and isinstance(e, dict) and e.get("polygons") is not None:
            if has_rle(e):
                sizes.add((int(e["mask"]["size"][0]), int(e["mask"]["size"][1])))
        elif masks_from == "polygons" and not has_rle(e):
            raise ValueError(f"{path}: entry {j} of {stem} has neither \"polygons\" nor a \"mask\" RLE: nothing to rebuild it from")
        elif not has_rle(e):
            raise ValueError(f"{path}: entry {j} has no \"mask\" RLE (written with --no-rle?): nothing to rebuild it from")
        else:
            sizes.add((int(e["mask"]["size"][0]), int(e["mask"]["size"][1])))
        label = int(e["label"])
        if not 0 <= label < n_classes:
            raise ValueError(f"{path}: entry {j} holds label {label}, outside 0..{n_classes - 1}: it was written with another class "
                             "list (use the same --classes / --n-classes)")
    if len(sizes) > 1:
        raise ValueError(f"{path}: the entries' masks have mixed sizes {sorted(sizes)}")
    return entries, (next(iter(sizes)) if sizes else None)


class Relabeler:
    """The device side: one image's entries in, its outputs out.  Holds the buffers that are reused from image to image."""

    def __init__(self, engine, n_classes: int, palette: np.ndarray, args):
        self.eng, self.dev = engine, engine.device
        self.box_batch = int(args.box_batch)
        self.min_region_area, self.region_mode = int(args.min_region_area or 0), args.region_mode
        self.resolve = args.overlap != "order"
        self.overlap = args.overlap
        self.mask_boxes = bool(args.mask_boxes or args.dota_txt)
        self.polygon_eps_q = polygon_eps_q(float(getattr(args, "polygon_epsilon", 0.0) or 0.0))
        self.polygons = bool(args.polygons) or self.polygon_eps_q > 0
        self.polygon_max_edges, self.polygon_buffer_mb = int(args.polygon_max_edges), int(args.polygon_buffer_mb)
        self.rle_buffer_mb = int(args.rle_buffer_mb)
        self.polygon_iou = bool(getattr(args, "polygon_iou", False))
        self.masks_from = getattr(args, "masks_from", "rle") or "rle"
        if self.masks_from not in MASK_SOURCES:
            raise ValueError(f"masks_from must be one of {list(MASK_SOURCES)}, got {self.masks_from!r}")
        lut, poly_vertices = validate_output_options(self.min_region_area, self.region_mode, self.polygons, self.polygon_buffer_mb,
                                                     self.polygon_max_edges, tile_io.class_lut(palette) if args.png_device else None,
                                                     "smallest" if self.resolve else "order", self.polygon_eps_q / 16.0, self.polygon_iou)
        self.png_lut = None if lut is None else torch.from_numpy(np.ascontiguousarray(lut)).to(self.dev)
        self.class_pixels = torch.zeros(n_classes, dtype=torch.int64, device=self.dev)
        self.class_instances = torch.zeros(n_classes, dtype=torch.int64, device=self.dev)
        self.rle_dev = torch.empty(self.rle_buffer_mb << 20, dtype=torch.uint8, device=self.dev)
        if self.polygons:
            self.poly_vert = torch.empty(poly_vertices, 2, dtype=torch.int32, device=self.dev)
            self.poly_ring = torch.empty(poly_vertices // 4, 4, dtype=torch.int32, device=self.dev)
        self.png_dev = None

    @torch.no_grad()
    def image(self, path: str, entries: List[dict], size: Tuple[int, int]) -> Dict:
        """One image's entries through the chain -> what ``generate.write_outputs`` takes (host arrays)."""
        eng, dev, (H, W), n = self.eng, self.dev, size, len(entries)
        i64 = dict(dtype=torch.int64, device=dev)
        seg = torch.full((H, W), 255, dtype=torch.uint8, device=dev)
        labels = torch.tensor([int(e["label"]) for e in entries], dtype=torch.int32, device=dev)
        areas, status = torch.zeros(n, **i64), torch.zeros(n, dtype=torch.int32, device=dev)
        changed = torch.zeros(n, **i64) if self.min_region_area else None
        removed = torch.zeros(n, **i64) if self.resolve else None
        hbox = rbox = rec = None
        if self.mask_boxes:
            hbox, rbox = torch.zeros(n, 4, dtype=torch.int32, device=dev), torch.zeros(n, 4, 2, dtype=torch.float32, device=dev)
            rec = torch.zeros(n, 8, **i64)
        ptab = pcur = pcnt = None
        if self.polygons:
            ptab, pcur = torch.zeros(n, 5, **i64), torch.zeros(2, **i64)
            pcnt = torch.zeros(n, 3, **i64) if self.polygon_iou else None
        rtab, rcur = torch.zeros(n, 3, **i64), torch.zeros(1, **i64)
        # --masks-from polygons: the entries that carry rings are filled on the device; the others (not traced) keep their RLE
        from_rings = [self.masks_from == "polygons" and e.get("polygons") is not None for e in entries]
        coded = [j for j in range(n) if not from_rings[j]]
        if coded:
            # one upload: the table, then the strings
            buf, table = rle.pack_strings([entries[j]["mask"] for j in coded])
            both = torch.from_numpy(np.concatenate([table.reshape(-1).view(np.uint8), buf])).to(dev)
            strings, table = both[table.size * 8:], both[:table.size * 8].view(torch.int64).view(-1, 3)
        filled = torch.zeros(n, 3, **i64)                         # --masks-from polygons: the fill's counts of the entries with rings
        row_of = {j: k for k, j in enumerate(coded)}              # entry -> its row of the uploaded string table
        # the overlap stage needs every mask of the image at once: one chunk
        for s, e in ([(0, n)] if n else []) if self.resolve else box_chunks(n, self.box_batch):
            if not any(from_rings[s:e]):
                masks, _, _ = eng.rle_decode(strings, table[row_of[s]:row_of[s] + e - s], (H, W), status_out=status[s:e])
            else:
                t, r, v = pack_rings([[np.asarray(p) for p in entries[j]["polygons"]] if from_rings[j] else None for j in range(s, e)])
                masks, _ = eng.fill_polygons(torch.from_numpy(t).to(dev), torch.from_numpy(r).to(dev), torch.from_numpy(v).to(dev),
                                             (H, W), counts_out=filled[s:e])        # [:, 0] == -1: rings that cannot be filled
                for j in range(s, e):                              # rare: a mask over the edge cap among traced ones
                    if not from_rings[j]:
                        eng.rle_decode(strings, table[row_of[j]:row_of[j] + 1], (H, W), out=masks[j - s:j - s + 1],
                                       status_out=status[j:j + 1])
            if self.min_region_area:
                eng.clean_masks(masks, self.min_region_area, self.region_mode, areas_out=False, changed_out=changed[s:e])
            if self.resolve:
                eng.resolve_overlaps(masks, self.overlap, low=None, owner_out=False, before_out=False, removed_out=removed[s:e])
            if self.mask_boxes:
                eng.mask_boxes(masks, (0, 0), hbox[s:e], rbox[s:e], rec[s:e])
            if self.polygons:
                eng.mask_polygons(masks, (0, 0), self.polygon_max_edges, self.poly_vert, self.poly_ring, pcur, ptab[s:e])
                if self.polygon_iou:                                       # while the chunk's masks are here: its rows, simplified now
                    if self.polygon_eps_q:
                        eng.simplify_polygons(ptab[s:e], self.poly_ring, self.poly_vert, pcur, self.polygon_eps_q / 16.0)
                    eng.fill_polygons(ptab[s:e], self.poly_ring, self.poly_vert, (H, W), out=False, ref=masks, counts_out=pcnt[s:e])
            eng.paint(masks, labels[s:e], seg, self.class_pixels, self.class_instances, areas_out=areas[s:e])
            eng.rle_encode(masks, self.rle_dev, rcur, rtab[s:e])
        if self.polygons and self.polygon_eps_q and n and not self.polygon_iou:    # the image's rings, once, after its last chunk
            eng.simplify_polygons(ptab, self.poly_ring, self.poly_vert, pcur, self.polygon_eps_q / 16.0)
        png_tab = None
        if self.png_lut is not None:
            need = 6 << 20 if H * W <= (1 << 20) else 6 * H * W
            if self.png_dev is None or self.png_dev.numel() < need:
                self.png_dev = torch.empty(need, dtype=torch.uint8, device=dev)
            png_tab, png_cur = torch.zeros(1, 2, 2, **i64), torch.zeros(1, **i64)
            eng.png_encode(seg, self.png_lut, self.png_dev, png_cur, png_tab)
        status = status.cpu().numpy()                                      # synchronises: everything above is done
        bad = np.flatnonzero(status)
        if bad.size:
            raise ValueError(f"{path}: the \"mask\" of entry {int(bad[0])} does not decode: {RLE_STATUS[int(status[bad[0]])]}"
                             + (f" ({bad.size - 1} more entries)" if bad.size > 1 else ""))
        unfilled = [j for j in np.flatnonzero(filled[:, 0].cpu().numpy() < 0) if from_rings[j]]
        if unfilled:
            raise ValueError(f"{path}: the \"polygons\" of entry {int(unfilled[0])} cannot be filled: a vertex lies farther than 2^20 from "
                             "the image's origin" + (f" ({len(unfilled) - 1} more entries)" if len(unfilled) > 1 else ""))
        rtab, used = rtab.cpu().numpy(), int(rcur.item())
        check_packed(rtab, used, "image", self.rle_buffer_mb)
        data = self.rle_dev[:used].cpu().numpy()
        out = {"seg": seg.cpu().numpy(), "areas": areas.cpu().numpy(), "png_files": None, "mask_bboxes": None, "mask_rboxes": None,
               "polygons": None, "polygon_counts": None if pcnt is None else pcnt.cpu().numpy(), "removed": None if removed is None else removed.cpu().numpy(),
               "changed": None if changed is None else changed.cpu().numpy(),
               "rles": [{"size": [int(H), int(W)], "counts": data[int(o):int(o) + int(l)].tobytes().decode("ascii")} for o, l, _ in rtab]}
        if png_tab is not None:
            t = png_tab.cpu().numpy().reshape(2, 2)
            check_packed(t, 0, "image", self.png_dev.numel() >> 20, what="PNG buffer too small: a file", knob="the PNG buffer")
            files = self.png_dev[:int(t[:, 0].max() + t[:, 1].max())].cpu().numpy()
            out["png_files"] = tuple(files[int(o):int(o) + int(l)].tobytes() for o, l in t)
        if self.mask_boxes:
            hb, rb, rc = hbox.cpu().numpy(), rbox.cpu().numpy(), rec.cpu().numpy()
            # COCO [x, y, w, h] of whole pixels, None for an empty mask (driver.TileResult.mask_bbox)
            out["mask_bboxes"] = [None if int(rc[j, 6]) == 0 else [int(hb[j, 0]), int(hb[j, 1]), int(hb[j, 2] - hb[j, 0] + 1),
                                                                    int(hb[j, 3] - hb[j, 1] + 1)] for j in range(n)]
            out["mask_rboxes"] = [None if bb is None else rb[j].copy() for j, bb in enumerate(out["mask_bboxes"])]
        if self.polygons:
            tab, (nv, nr) = ptab.cpu().numpy(), (int(v) for v in pcur.cpu().numpy())
            check_polygons(tab, nv, nr, "image", self.polygon_buffer_mb)
            vert, ring = self.poly_vert[:nv].cpu().numpy(), self.poly_ring[:nr].cpu().numpy()
            out["polygons"] = [rings_of(tab, ring, vert, j) for j in range(n)]
        return out


def run(args) -> Dict:
    import samrs_amd
    why = refusal(args)
    if why:
        raise ValueError(why)
    names = [l.strip() for l in open(args.classes)] if args.classes else [str(i) for i in range(args.n_classes)]
    n_classes = len(names)
    palette = np.load(args.palette) if args.palette else generate.default_palette(n_classes)
    if n_classes > 255 or len(palette) > 255:
        raise ValueError(f"{n_classes} classes / {len(palette)} palette rows: class ids must stay below 255 (255 = unlabeled)")
    ins = ins_dir_of(args.ins)
    stems = sorted(f[:-4] for f in os.listdir(ins) if f.endswith(".pkl"))
    n_all = len(stems)
    done_before: List[str] = []
    if args.resume:
        done_before = [s for s in stems if generate.outputs_exist(args.out, s)]
        keep = set(done_before)
        stems = [s for s in stems if s not in keep]
        print(f"--resume: {len(done_before)} of {n_all} images already complete", flush=True)
    old_pix, old_ins, old_sizes = generate.resumed_statistics(args.out, done_before, n_classes)
    tile_io.load_library()
    torch.cuda.set_device(0)
    sam = samrs_amd.sam_model_registry[args.model](max_prompts=1).to("cuda:0")
    work = Relabeler(sam.engine, n_classes, palette, args)
    dota_txt = bool(args.dota_txt)
    sizes: List[int] = []
    cleaned, resolved = [0, 0], [0, 0]
    piou = PolygonIoUStat()
    for stem in stems:
        path = os.path.join(ins, stem + ".pkl")
        entries, size = load_entries(path, n_classes, work.masks_from)
        if size is None:
            # no instance (or none with an RLE), no size: a generate output directory still has the map's
            gray = os.path.join(os.path.dirname(os.path.abspath(ins)), "gray", stem + ".png")
            if not os.path.exists(gray):
                raise ValueError(f"{path}: no entry says the image's size (and there is no {gray} to take it from)")
            size = tuple(int(v) for v in tile_io.png_size(gray))
        r = work.image(path, entries, size)
        labels = np.array([int(e["label"]) for e in entries], dtype=np.int64)
        generate.write_outputs(args.out, stem, r["seg"], None, [e.get("bbox") for e in entries], labels, r["areas"], palette, names,
                               r["rles"], None, args.png_level, r["png_files"], r["mask_bboxes"], r["mask_rboxes"], dota_txt, None,
                               r["polygons"], r["removed"], None, base_entries=entries,
                               polygon_epsilon=work.polygon_eps_q / 16.0 if work.polygon_eps_q else None,
                               polygon_ious=None if r["polygon_counts"] is None else
                               [None if c[0] < 0 else float(iou_from_counts(c)) for c in r["polygon_counts"]])
        if r["polygon_counts"] is not None:
            piou.add(r["polygon_counts"])
        sizes.extend(int(a) for a in r["areas"] if a > 0)                                          # statistic.py:44-49
        if r["changed"] is not None:
            cleaned[0] += int(r["changed"].sum())
            cleaned[1] += int((r["changed"] > 0).sum())
        if r["removed"] is not None:
            resolved[0] += int(r["removed"].sum())
            resolved[1] += int((r["removed"] > 0).sum())
    pix = work.class_pixels.cpu().numpy() + old_pix
    inst = work.class_instances.cpu().numpy() + old_ins
    all_sizes = old_sizes + sizes
    stats = {"class_pixel_num": pix.tolist(), "class_instance_num": inst.tolist(), "mask_num": len(all_sizes)}
    if work.min_region_area > 0:
        stats["region_cleanup"] = {"min_region_area": work.min_region_area, "region_mode": args.region_mode,
                                   "changed_pixel_num": cleaned[0], "changed_instance_num": cleaned[1]}
    if work.resolve:
        stats["overlap"] = {"rule": args.overlap, "removed_pixel_num": resolved[0], "removed_instance_num": resolved[1]}
    stats["source"] = "ins"
    os.makedirs(os.path.join(args.out, "statistic"), exist_ok=True)
    with open(os.path.join(args.out, "statistic", "class_stats.json"), "w") as f:
        json.dump(stats, f)
    np.save(os.path.join(args.out, "statistic", "all_mask_size.npy"), np.asarray(all_sizes, dtype=np.int64))
    if work.polygon_iou:
        with open(os.path.join(args.out, "statistic", "polygon_iou.json"), "w") as f:
            json.dump(reduce_polygon_iou(piou, work.polygon_eps_q / 16.0), f)
    return stats


def main(argv=None):
    run(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
