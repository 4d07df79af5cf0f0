"""Scene mode: hbox -> semantic labels for images larger than the encoder's input, decoded window by window.

Every other path of this package treats one input image as one SAM image (the reference does too,
``Generate Dataset/main_sam_hbox_semantic.py:155``): a 4096^2 scene is resized to 1024^2 and a 16 px vehicle reaches the encoder
as 4 px.  Here the scene stays on the device at full resolution, ``plan_scene`` assigns every box to exactly ONE window (a cell of
an overlapping grid, or a context window of its own when no cell holds it), the windows are encoded `batch` at a time as crops of
the resident scene, each window's boxes are decoded against its embedding, and the masks are composited in the scene's own frame
on the device:

* ``Engine.scene_claim``        keeps, per scene pixel, the highest annotation rank whose mask is set there -- the reference's
                                "later box wins" (main_sam_hbox_semantic.py:195-199) across windows, whatever order they run in;
* ``Engine.scene_resolve``      turns that map into the class map once all windows are in;
* ``Engine.rle_encode_placed``  writes each mask's COCO RLE with ``size = [H, W]`` without an n x H x W stack ever existing.

Scene mode is off unless asked for (``samrs_amd.generate --scene-window``); nothing else in the package calls into this module.
"""
from __future__ import annotations

import math
import time
import warnings
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import numpy as np

Window = Tuple[int, int, int, int]          # (x0, y0, w, h), inside the scene


def axis_spans(L: int, window: int, overlap: int) -> List[Tuple[int, int]]:
    """Rule 1: (start, length) of the grid along an axis of length L -- the DOTA split rule (the last window is shifted in,
    not padded)."""
    if L <= window:
        return [(0, L)]
    step = window - overlap
    starts, s = [], 0
    while s + window < L:
        starts.append(s)
        s += step
    starts.append(L - window)
    return [(s, window) for s in starts]


def box_hull(box, H: int, W: int) -> Tuple[int, int, int, int]:
    """Rule 2: the box clipped to [0, W] x [0, H], then its integer hull (lx, ly, hx, hy)."""
    x1, y1, x2, y2 = (float(v) for v in box)
    x1, x2 = min(max(x1, 0.0), float(W)), min(max(x2, 0.0), float(W))
    y1, y2 = min(max(y1, 0.0), float(H)), min(max(y2, 0.0), float(H))
    return int(math.floor(x1)), int(math.floor(y1)), int(math.ceil(x2)), int(math.ceil(y2))


def window_contains(win: Window, hull) -> bool:
    x0, y0, w, h = win
    lx, ly, hx, hy = hull
    return x0 <= min(lx, hx) and max(lx, hx) <= x0 + w and y0 <= min(ly, hy) and max(ly, hy) <= y0 + h


def plan_scene(H: int, W: int, boxes, window: int = 1024, overlap: int = 256, context: float = 2.0):
    """Which window each box of an H x W scene is decoded in -> (windows, window_of): `windows` a list of (x0, y0, w, h) int
    tuples inside the scene, in order of first use, `window_of[j]` the index of box j's window.  Deterministic; every box gets
    exactly one window, and that window contains the box's clipped integer hull.

    1. grid along each axis (``axis_spans``), windows = the row-major product, y outer;
    2. a box is clipped to the scene and widened to its integer hull (``box_hull``);
    3. of the grid windows that contain the hull the one with the greatest margin min(lx-x0, ly-y0, x0+w-hx, y0+h-hy) holds the
       box, ties to the first in grid order;
    4. a box no grid window contains (larger than the window, or straddling by more than the overlap) gets a context window of
       side max(window, ceil(context * its longer side)), cut to the scene, centred on the hull and shifted inside the scene;
    5. only windows that hold a box are emitted, identical ones once."""
    H, W, window, overlap = int(H), int(W), int(window), int(overlap)
    if H < 1 or W < 1 or window < 1:
        raise ValueError("scene and window sizes must be positive")
    if not 0 <= overlap < window:
        raise ValueError(f"overlap must satisfy 0 <= overlap < window, got overlap={overlap}, window={window}")
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    xs, ys = axis_spans(W, window, overlap), axis_spans(H, window, overlap)
    grid = [(x0, y0, w, h) for (y0, h) in ys for (x0, w) in xs]
    windows: List[Window] = []
    index = {}
    window_of: List[int] = []
    for box in boxes:
        lx, ly, hx, hy = hull = box_hull(box, H, W)
        best, best_margin = None, None
        for win in grid:
            if not window_contains(win, hull):
                continue
            x0, y0, w, h = win
            margin = min(lx - x0, ly - y0, x0 + w - hx, y0 + h - hy)
            if best is None or margin > best_margin:
                best, best_margin = win, margin
        if best is None:
            s = max(window, int(math.ceil(context * max(hx - lx, hy - ly))))
            w, h = min(s, W), min(s, H)
            cx, cy = (lx + hx) // 2, (ly + hy) // 2
            best = (min(max(cx - w // 2, 0), W - w), min(max(cy - h // 2, 0), H - h), w, h)
        if best not in index:
            index[best] = len(windows)
            windows.append(best)
        window_of.append(index[best])
    return windows, window_of


class ScenePipeline:
    """hbox -> semantic labels for a stream of scenes of any size; takes the ``WorkItem`` s of ``TilePipeline`` (boxes in scene
    pixels, annotation order) and hands ``TileResult`` s to the sink: ``seg_mask`` [H, W], ``areas`` / ``boxes`` / ``labels`` in the
    caller's order, RLE with ``size = (H, W)`` when `rle`, device PNGs of the scene map with `png_lut`, and the plan in
    ``windows`` / ``window_of``.  Scenes run one after the other; within a scene the encoder pass of the next `batch` windows runs
    on a stream of its own beside the decoding and compositing of the current ones when the engine has two sets of embedding slots
    (``max_images >= 2 * batch``).  The results do not depend on `batch` (windows per encoder pass) or `box_batch` (prompts per
    decoder call).  A scene no larger than `window` is one window, and every
    output equals ``TilePipeline``'s for the same item byte for byte.  `mask_boxes`: each mask's tight hbox, minimum-area rotated
    box and record (``Engine.mask_boxes``) with its window's origin as the offset, so they are in the scene's frame, exactly:
    ``TileResult.mask_hbox`` / ``mask_rbox`` / ``mask_record``; off (default) launches and allocates nothing.  `polygons`: each
    mask's outline as polygons on the pixel lattice (``Engine.mask_polygons``), again with the window's origin as the offset, so the
    vertices are in the scene's frame exactly: ``TileResult.polygons(j)``; `polygon_buffer_mb` holds one scene's vertices and ring
    records (an overflow raises, naming it), a mask over `polygon_max_edges` edges yields None; off launches and allocates nothing.
    `polygon_epsilon` > 0 (pixels; needs `polygons`): the scene's rings are simplified once, on the device, after the last window
    (``Engine.simplify_polygons``; ``driver.polygon_eps_q``), in the scene's frame like the rings themselves; 0.0 makes no call."""

    def __init__(self, sam, n_classes: int, window: int = 1024, overlap: int = 256, context: float = 2.0, batch: int = 8,
                 box_batch: int = 64, rle: bool = False, png_lut: Optional[np.ndarray] = None, min_region_area: int = 0,
                 region_mode: str = "both", precision="auto", rle_buffer_mb: int = 256, mask_boxes: bool = False,
                 quality: bool = False, min_stability: float = 0.0, min_pred_iou: float = 0.0, min_inside_box: float = 0.0,
                 polygons: bool = False, polygon_buffer_mb: int = 64, polygon_max_edges: int = 65536, vis_lut=None, boundary: bool = False,
                 polygon_epsilon: float = 0.0, polygon_iou: bool = False):
        import torch
        from .driver import (TilePipeline, output_tables, polygon_eps_q, refuse_boundary_option, refuse_overlap_option,
                             refuse_polygon_iou_option, refuse_quality_options, refuse_vis_option, validate_output_options)
        refuse_polygon_iou_option("ScenePipeline", "a window's masks are gone when the scene's rings are simplified; not built",
                                  polygon_iou=polygon_iou)
        refuse_boundary_option("ScenePipeline", "scenes carry no ground truth; Boundary AP across windows is not built", boundary=boundary)
        refuse_vis_option("ScenePipeline", "the scene's composite lives in another buffer; scene overlays are not built", vis_lut=vis_lut)
        if isinstance(overlap, str):        # TilePipeline's overlap rule; the name means the windows' overlap in pixels here
            refuse_overlap_option("ScenePipeline", "resolving across scene windows is not built", overlap=overlap)
            raise ValueError("ScenePipeline's overlap is the windows' overlap in pixels; masks always overlap in painting order here")
        refuse_quality_options("ScenePipeline", "scoring across scene windows is not built", quality=quality,
                               min_stability=min_stability, min_pred_iou=min_pred_iou, min_inside_box=min_inside_box)
        from .transforms import ResizeLongestSide
        if not 0 <= int(overlap) < int(window):
            raise ValueError(f"overlap must satisfy 0 <= overlap < window, got overlap={overlap}, window={window}")
        lut, nv = validate_output_options(min_region_area, region_mode, polygons, polygon_buffer_mb, polygon_max_edges, png_lut,
                                          polygon_epsilon=polygon_epsilon)
        self.polygon_eps_q = polygon_eps_q(polygon_epsilon, bool(polygons))
        eng = sam.engine
        if eng is None:
            raise RuntimeError("move the model to the GPU first: sam.to('cuda')")
        if eng.max_images < batch:
            raise ValueError(f"ScenePipeline(batch={batch}) needs an engine with max_images >= {batch}; got {eng.max_images}")
        if box_batch > eng.max_prompts:
            raise ValueError(f"ScenePipeline(box_batch={box_batch}) needs an engine with max_prompts >= {box_batch}; got {eng.max_prompts}")
        self.sam, self.eng, self.dev = sam, eng, eng.device
        self.window, self.overlap, self.context = int(window), int(overlap), float(context)
        self.batch, self.box_batch, self.rle = int(batch), int(box_batch), bool(rle)
        self.min_region_area, self.region_mode = int(min_region_area), region_mode
        self.mask_boxes = bool(mask_boxes)
        self.polygons = bool(polygons)
        self.tables = output_tables(self.min_region_area, self.mask_boxes)      # per scene: one device table of n rows each
        if self.polygons:
            self.polygon_buffer_mb, self.polygon_max_edges = int(polygon_buffer_mb), int(polygon_max_edges)
            self.poly_vert_dev = torch.empty(nv, 2, dtype=torch.int32, device=eng.device)
            self.poly_ring_dev = torch.empty(nv // 4, 4, dtype=torch.int32, device=eng.device)
        # the operand-split mode of this pipeline's own calls: TilePipeline's rule and TilePipeline's scoping
        self.split_mode = TilePipeline._choose_split(sam, precision, multimask=False)
        self.allow_reduced = False
        self._mode = lambda: TilePipeline._mode(self)
        if self.split_mode is not None:
            with self._mode():
                pass
        self.side = sam.cfg.img_size
        self.transform = ResizeLongestSide(sam.image_encoder.img_size)
        self.s_enc = torch.cuda.Stream(self.dev)
        self.ev_enc = [torch.cuda.Event() for _ in range(2)]
        self.ev_dec = [torch.cuda.Event() for _ in range(2)]
        self.class_pixels = torch.zeros(n_classes, dtype=torch.int64, device=self.dev)
        self.class_instances = torch.zeros(n_classes, dtype=torch.int64, device=self.dev)
        self.png = png_lut is not None
        self._png_warned = False
        # stage_seconds = {} switches on a host clock per stage (upload / windows / finish), each closed by a device synchronise:
        # for tools/scene_bench.py's attribution run only -- the synchronises cost throughput
        self.stage_seconds: Optional[dict] = None
        if self.png:
            self.png_lut = torch.from_numpy(lut).to(self.dev)
            self.png_dev = None
        if self.rle:
            self.rle_buffer_mb = int(rle_buffer_mb)
            self.rle_dev = torch.empty(self.rle_buffer_mb << 20, dtype=torch.uint8, device=self.dev)

    # samrs_png_encode_labels' stated limit (include/samrs_hip.h)
    @staticmethod
    def png_device_ok(H: int, W: int) -> bool:
        return H <= 65536 and W <= 65536 and (3 * W + 1) * H < 2 ** 31

    def _encode_windows(self, scene, group: Sequence[Window], slot0: int):
        """One encoder pass over the windows of `group` (crops of the resident scene) into slots slot0 .. slot0 + len(group) - 1, on
        the current stream; returns each window's input size.  A crop that is not side x side goes through the PIL-exact device
        resize and the ragged entry point, exactly as TilePipeline._stage / _encode do for a tile of that size."""
        import torch
        tiles, native = [], True
        for (x0, y0, w, h) in group:
            t = scene[y0:y0 + h, x0:x0 + w].contiguous()
            if (h, w) != (self.side, self.side):
                t = self.transform.apply_image_device(t)
                native = False
            tiles.append(t)
        with self._mode():
            if native:
                self.eng.set_images(torch.stack(tiles), slot0)
            else:
                self.eng.set_images_ragged(tiles, slot0)
        return [(int(t.shape[0]), int(t.shape[1])) for t in tiles]

    def _run_scene(self, it):
        import torch
        from .driver import TileResult, box_chunks, check_packed, check_polygons
        eng, dev = self.eng, self.dev
        t_stage = [time.perf_counter()]

        def stage(name):
            if self.stage_seconds is not None:
                torch.cuda.synchronize(dev)
                now = time.perf_counter()
                self.stage_seconds[name] = self.stage_seconds.get(name, 0.0) + now - t_stage[0]
                t_stage[0] = now
        img = it.image
        if isinstance(img, torch.Tensor):
            scene = img.to(dev).contiguous()
        else:
            scene = torch.from_numpy(np.ascontiguousarray(img)).to(dev)                     # the scene crosses PCIe once
        H, W = int(scene.shape[0]), int(scene.shape[1])
        boxes = np.asarray(it.boxes, dtype=np.float32).reshape(-1, 4)
        labels = np.asarray(it.labels).astype(np.int32).reshape(-1)
        n = len(labels)
        windows, window_of = plan_scene(H, W, boxes, self.window, self.overlap, self.context)
        # boxes, labels and ranks in WINDOW order (window by window, annotation order inside a window), one upload each: a window's
        # prompts and the rows of its results are then contiguous slices.  The shift by the window origin is one fp32 subtraction
        # per coordinate (x - 0.0f == x bit for bit for a window at the origin)
        wo = np.asarray(window_of, dtype=np.int64)
        perm = np.argsort(wo, kind="stable")
        first = np.searchsorted(wo[perm], np.arange(len(windows) + 1))
        origin = np.asarray([(x0, y0, x0, y0) for (x0, y0, _, _) in windows], dtype=np.float32).reshape(-1, 4)
        dev_perm = torch.from_numpy(perm).to(dev)
        w_box = torch.from_numpy(boxes[perm]).to(dev) - torch.from_numpy(origin[wo[perm]]).to(dev)
        w_lab = torch.from_numpy(labels[perm]).to(dev)
        w_rank = dev_perm.to(torch.int32)
        order = torch.full((H, W), -1, dtype=torch.int32, device=dev)
        tabs = {t.field: t.alloc(1, n, dev)[0] for t in self.tables}        # the per-box tables, rows in window order
        if self.polygons:
            w_ptab = torch.zeros(n, 5, dtype=torch.int64, device=dev)
            poly_cur = torch.zeros(2, dtype=torch.int64, device=dev)
        if self.rle:
            w_tab = torch.zeros(n, 3, dtype=torch.int64, device=dev)
            rle_cur = torch.zeros(1, dtype=torch.int64, device=dev)
        # the encoder pass of group g + 1 runs on its own stream while group g is decoded and composited on the caller's, when the
        # engine has a second set of embedding slots for it (max_images >= 2 * batch); otherwise the two take turns
        stage("upload")
        cur = torch.cuda.current_stream(dev)
        two = eng.max_images >= 2 * self.batch
        groups = [windows[g:g + self.batch] for g in range(0, len(windows), self.batch)]
        in_sizes = [None] * len(groups)
        self.s_enc.wait_stream(cur)
        scene.record_stream(self.s_enc)

        def encode(g):
            b = g & 1 if two else 0
            with torch.cuda.stream(self.s_enc):
                self.s_enc.wait_event(self.ev_dec[b])                   # the decoder is done with slot set b
                in_sizes[g] = self._encode_windows(scene, groups[g], b * self.batch)
                self.ev_enc[b].record(self.s_enc)

        if groups:
            encode(0)
        for g, group in enumerate(groups):
            b = g & 1 if two else 0
            if two and g + 1 < len(groups):
                encode(g + 1)
            cur.wait_event(self.ev_enc[b])
            for i, win in enumerate(group):
                x0, y0, w, h = win
                k = g * self.batch + i
                p0, p1 = int(first[k]), int(first[k + 1])
                for s, e in box_chunks(p1 - p0, self.box_batch):
                    s, e = p0 + s, p0 + e
                    tb = w_box[s:e] if (h, w) == in_sizes[g][i] else self.transform.apply_boxes_torch(w_box[s:e], (h, w))
                    with self._mode():
                        masks, _, _ = eng.predict(b * self.batch + i, tb, None, None, None, False, False, in_sizes[g][i], (h, w))
                    m = masks[:, 0]
                    if self.min_region_area:                                      # before anything else reads the masks
                        eng.clean_masks(m, self.min_region_area, self.region_mode, areas_out=False, changed_out=tabs["changed"][s:e])
                    if self.mask_boxes:                                           # in the scene's frame: the window's origin
                        eng.mask_boxes(m, (x0, y0), tabs["mask_hbox"][s:e], tabs["mask_rbox"][s:e], tabs["mask_record"][s:e])
                    if self.polygons:                                             # lattice vertices in the scene's frame
                        eng.mask_polygons(m, (x0, y0), self.polygon_max_edges, self.poly_vert_dev, self.poly_ring_dev, poly_cur,
                                          w_ptab[s:e])
                    eng.scene_claim(m, w_rank[s:e], win, order, w_lab[s:e], self.class_pixels, self.class_instances,
                                    areas_out=tabs["areas"][s:e])
                    if self.rle:
                        eng.rle_encode_placed(m, win, (H, W), self.rle_dev, rle_cur, w_tab[s:e])
            self.ev_dec[b].record(cur)
            if not two and g + 1 < len(groups):
                encode(g + 1)
        if self.polygons and self.polygon_eps_q and n:             # the scene's rings, once; the rows are in placement (window) order
            eng.simplify_polygons(w_ptab, self.poly_ring_dev, self.poly_vert_dev, poly_cur, self.polygon_eps_q / 16.0)
        stage("windows")
        dev_lab = torch.from_numpy(labels).to(dev)

        def unpermute(t):                                       # window order -> the caller's order
            out = np.empty_like(t)
            out[perm] = t
            return out
        seg = eng.scene_resolve(order, dev_lab)
        png_tab = None
        if self.png:
            if self.png_device_ok(H, W):
                need = 16 + 6 * H * W + (1 << 16)                  # TilePipeline's 6 MiB per 1024^2 map: two all-literal files fit
                if self.png_dev is None or self.png_dev.numel() < need:
                    self.png_dev = torch.empty(need, dtype=torch.uint8, device=dev)
                png_cur = torch.zeros(1, dtype=torch.int64, device=dev)
                png_tab = torch.zeros(1, 2, 2, dtype=torch.int64, device=dev)
                eng.png_encode(seg, self.png_lut, self.png_dev, png_cur, png_tab)
            elif not self._png_warned:
                self._png_warned = True
                warnings.warn(f"scene {it.key!r} ({H} x {W}) exceeds the device PNG encoder's limit; this and any later such scene "
                              "carry no device PNG (TileResult.png_table is None): write them with tile_io.write_label_pair")
        r = TileResult(it.key, seg.cpu().numpy(), boxes=np.asarray(it.boxes), labels=np.asarray(it.labels),
                       **{f: unpermute(t.cpu().numpy()) for f, t in tabs.items()})
        r.size = (H, W)
        r.windows, r.window_of = windows, window_of
        if self.polygons:
            ptab = unpermute(w_ptab.cpu().numpy())
            nv, nr = (int(v) for v in poly_cur.cpu().tolist())
            check_polygons(ptab, nv, nr, "scene", self.polygon_buffer_mb)
            r.polygon_table = ptab
            r.polygon_rings, r.polygon_vertices = self.poly_ring_dev[:nr].cpu().numpy(), self.poly_vert_dev[:nv].cpu().numpy()
        if self.rle:
            tab = unpermute(w_tab.cpu().numpy())
            total = int(rle_cur.item())
            check_packed(tab, total, "scene", self.rle_buffer_mb)
            r.rle_table, r.rle_data = tab, self.rle_dev[:total].cpu().numpy()
        if png_tab is not None:
            t = png_tab.cpu().numpy()[0]
            if int(t[:, 1].min()) < 0:
                raise RuntimeError("PNG buffer too small for the scene's class map")
            r.png_table, r.png_data = t, self.png_dev[:int(png_cur.item())].cpu().numpy()
        stage("finish")
        return r

    def run(self, items: Iterable, sink: Callable[[List, Callable[[], None]], None]) -> int:
        """Drives `items` (``WorkItem`` s, one scene each) through the pipeline; `sink(results, release)` is called on the calling
        thread once per scene with a one-element list, as ``TilePipeline.run`` calls it per batch (the arrays are the result's own:
        `release` is there for the shared signature and does nothing).  Returns the number of windows encoded."""
        import torch
        n_windows = 0
        with torch.no_grad():
            for it in items:
                r = self._run_scene(it)
                n_windows += len(r.windows)
                sink([r], lambda: None)
        return n_windows
