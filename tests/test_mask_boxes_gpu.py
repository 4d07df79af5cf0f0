"""GPU: samrs_mask_boxes (box_kernels.hip: row extents, then per mask the strict hull chains, every candidate edge and an exact
argmin) and its two kernels alone (samrs_k_mask_row_extents, samrs_k_mask_hull) against the host restatement tests/box_ref.py,
then the option through the three pipelines and the generation CLI.  Integer work on both sides up to one correctly rounded fp64
division per corner coordinate: every comparison is exact, the fp32 corners included.

Shapes: a lane of the extents kernel owns 16 bytes of a row and a wave owns a row, so 67 x 93 (odd: the byte path) and 70 x 272
(whole 16-byte segments: the 16-byte path), 1 x 1, 1 x 40, 40 x 1, 96 x 96, 130 x 130 and 1024 x 1024 (a full wave per row, one
point per thread of the hull kernel) cover both load paths, partial waves, and rows beyond one block of the hull kernel's scans."""
import functools
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from samrs_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N_CLASSES = 18


def _sam(name="vit_tiny", **kw):
    import samrs_amd
    return samrs_amd.sam_model_registry[name](**kw).to("cuda")


@pytest.fixture(scope="module")
def eng():
    sam = _sam(max_images=1, max_prompts=4)
    yield sam.engine


def _assert_boxes(got, want, what=""):
    for name, g, w in zip(("hbox", "rbox", "record"), got, want):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what} {name}: {g.dtype} {g.shape}"
        bad = [j for j in range(len(w)) if g[j].tobytes() != w[j].tobytes()]
        assert not bad, f"{what} {name}: masks {bad} differ, first: got {g[bad[0]].tolist()} want {w[bad[0]].tolist()}"


def _check(eng, masks: np.ndarray, offset=(0, 0), what=""):
    """extents, hull and boxes of the device against box_ref; returns the device's (hbox, rbox, record) as numpy."""
    d = torch.from_numpy(np.ascontiguousarray(masks)).cuda()
    ext = eng.mask_row_extents(d).cpu().numpy()
    verts, counts = eng.mask_hull(d, offset, cap=2048)
    got = eng.mask_boxes(d, offset)
    torch.cuda.synchronize()
    verts, counts = verts.cpu().numpy(), counts.cpu().numpy()
    for j in range(len(masks)):
        assert np.array_equal(ext[j], box_ref.row_extents(masks[j])), f"{what} mask {j}: row extents"
        v = box_ref.hull(masks[j], *offset)
        assert int(counts[j]) == len(v), f"{what} mask {j}: {int(counts[j])} hull vertices, want {len(v)}"
        assert [tuple(p) for p in verts[j, :len(v)].tolist()] == v, f"{what} mask {j}: hull vertices"
    want = box_ref.mask_boxes(masks, *offset)
    _assert_boxes(got, want, what)
    return tuple(g.cpu().numpy() for g in got)


@pytest.mark.parametrize("shape", [(5, 67, 93), (3, 70, 272)])
@pytest.mark.parametrize("density", [0.02, 0.5])
def test_random_masks_byte_path_and_16_byte_path(eng, shape, density):
    rng = np.random.default_rng(int(density * 100) + shape[2])
    masks = (rng.random(shape) < density).astype(np.uint8)
    masks[masks != 0] = rng.integers(1, 256, int(masks.sum()), dtype=np.uint8)        # any non-zero byte is a set pixel
    _check(eng, masks, what=f"{shape} p={density}")


def test_smallest_shapes_and_many_masks_in_one_call(eng):
    _check(eng, np.ones((1, 1, 1), np.uint8), what="1 x 1 set")
    _check(eng, np.zeros((1, 1, 1), np.uint8), what="1 x 1 unset")
    rng = np.random.default_rng(7)
    _check(eng, (rng.random((2, 1, 40)) < 0.3).astype(np.uint8), what="1 x 40")
    _check(eng, (rng.random((2, 40, 1)) < 0.3).astype(np.uint8), what="40 x 1")
    many = (rng.random((33, 20, 37)) < 0.1).astype(np.uint8)
    many[5] = 0
    _check(eng, many, what="33 masks")


def _constructed(side: int):
    yy, xx = np.mgrid[0:side, 0:side]
    out = {"empty": np.zeros((side, side), np.uint8), "full": np.ones((side, side), np.uint8)}
    one = np.zeros((side, side), np.uint8)
    one[side // 3, side - 2] = 1
    out["one pixel"] = one
    blk = np.zeros((side, side), np.uint8)
    blk[11:40, 17:70] = 1
    out["block"] = blk
    for deg in (7, 30, 45, 83):
        out[f"bar {deg}"] = box_ref.rotated_bar(side, deg, 0.8 * side, 0.15 * side)
    out["disk 90"] = box_ref.disk(side, 90)
    frame = np.zeros((side, side), np.uint8)
    frame[0, 5] = frame[side - 1, side - 9] = frame[side // 2, 0] = frame[7, side - 1] = 1
    out["first and last row and column"] = frame
    out["diagonal"] = np.eye(side, dtype=np.uint8)
    out["anti-diagonal"] = np.ascontiguousarray(np.eye(side, dtype=np.uint8)[:, ::-1])
    out["diamond"] = box_ref.diamond(side, side // 2 - 3)
    tips = box_ref.disk(side, side // 2).copy()
    tips[0, side // 2 + 3] = tips[side - 1, side // 2 - 5] = 1
    out["single pixel in the top and in the bottom row"] = tips
    return out


@pytest.mark.parametrize("side", [96, 130])
def test_constructed_masks(eng, side):
    shapes = _constructed(side)
    masks = np.stack(list(shapes.values()))
    hb, rb, rec = _check(eng, masks, what=f"{side} x {side} " + " | ".join(shapes))
    names = list(shapes)
    assert not rec[names.index("empty")].any() and not rb[names.index("empty")].any() and not hb[names.index("empty")].any()
    assert rec[names.index("one pixel"), 6] == 1 and rec[names.index("diagonal"), 6] == 2 and rec[names.index("full"), 6] == 4
    d = rec[names.index("diamond")]
    assert d[6] == 4 and d[0] == -d[1] and d[0] < 0                 # four equal rectangles: edge 0 (down the left side) wins
    assert hb[names.index("full")].tolist() == [0, 0, side - 1, side - 1]


def test_full_size_call(eng):
    rng = np.random.default_rng(3)
    ell = np.zeros((1024, 1024), np.uint8)
    ell[100:900, 200:330] = 1
    ell[770:900, 200:800] = 1
    masks = np.stack([box_ref.disk(1024, 1022), (rng.random((1024, 1024)) < 0.5).astype(np.uint8), ell])
    hb, rb, rec = _check(eng, masks, what="1024 x 1024")
    assert rec[0, 6] == 216                                         # the disk's hull


def test_offset_equals_the_reference_on_the_shifted_points(eng):
    rng = np.random.default_rng(11)
    masks = np.stack([box_ref.rotated_bar(96, 30, 70, 12), (rng.random((96, 96)) < 0.05).astype(np.uint8)])
    hb0, rb0, rec0 = _check(eng, masks)
    hb, rb, rec = _check(eng, masks, offset=(1000, 31000), what="offset (1000, 31000)")
    assert np.array_equal(hb - hb0, np.tile(np.array([1000, 31000, 1000, 31000], np.int32), (2, 1)))
    assert np.array_equal(rec[:, [0, 1, 6, 7]], rec0[:, [0, 1, 6, 7]])
    _check(eng, masks, offset=(32768 - 96, 32768 - 96), what="the largest offset")


def test_unaligned_base_takes_the_byte_path_and_agrees(eng):
    rng = np.random.default_rng(5)
    masks = (rng.random((3, 70, 272)) < 0.3).astype(np.uint8)
    buf = torch.zeros(masks.size + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + masks.size].view(3, 70, 272)
    view.copy_(torch.from_numpy(masks).cuda())
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    want = box_ref.mask_boxes(masks)
    _assert_boxes(eng.mask_boxes(view), want, "unaligned base")
    assert np.array_equal(eng.mask_row_extents(view).cpu().numpy(), np.stack([box_ref.row_extents(m) for m in masks]))


def test_bad_arguments_leave_the_outputs_untouched_and_null_outputs_are_skipped(eng):
    from samrs_amd import engine
    lib, h = eng.lib, eng.handle
    m = torch.ones(2, 8, 8, dtype=torch.uint8, device="cuda")
    hb = torch.full((2, 4), -7, dtype=torch.int32, device="cuda")
    rb = torch.full((2, 4, 2), -7.0, dtype=torch.float32, device="cuda")
    rec = torch.full((2, 8), -7, dtype=torch.int64, device="cuda")

    def call(masks, n, hh, ww, x0, y0, a=hb, b=rb, c=rec):
        rc = lib.samrs_mask_boxes(h, masks, n, hh, ww, x0, y0, None if a is None else a.data_ptr(), None if b is None else b.data_ptr(),
                                  None if c is None else c.data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    p = m.data_ptr()
    for args in ((p, -1, 8, 8, 0, 0), (None, 2, 8, 8, 0, 0), (p, 2, 0, 8, 0, 0), (p, 2, 8, 0, 0, 0), (p, 2, 8193, 8, 0, 0),
                 (p, 2, 8, 8193, 0, 0), (p, 2, 8, 8, 32761, 0), (p, 2, 8, 8, 0, 32761), (p, 2, 8, 8, -1, 0), (p, 2, 8, 8, 0, -1)):
        assert call(*args) == engine.ERR_BAD_ARG, args
    assert (hb == -7).all() and (rb == -7).all() and (rec == -7).all()
    assert call(p, 0, 8, 8, 0, 0) == engine.OK                      # n == 0 is a no-op
    assert (hb == -7).all() and (rb == -7).all() and (rec == -7).all()
    assert call(p, 2, 8, 8, 32760, 32760, None, None, None) == engine.OK
    assert call(p, 2, 8, 8, 0, 0, hb, None, None) == engine.OK      # NULL outputs are skipped
    assert hb.cpu().tolist() == [[0, 0, 7, 7]] * 2 and (rb == -7).all() and (rec == -7).all()
    assert call(p, 2, 8, 8, 0, 0, None, rb, rec) == engine.OK
    assert rec.cpu().tolist() == [[0, 7, 0, 49, -49, 0, 4, 98]] * 2
    # the Python conventions: a caller-owned slice, None or False per output
    tab = torch.full((2, 6, 4), -7, dtype=torch.int32, device="cuda")
    a, b, c = eng.mask_boxes(m, hbox_out=tab[1, 2:4], rbox_out=False)
    assert a.data_ptr() == tab[1, 2:4].data_ptr() and b is None and c.shape == (2, 8)
    assert tab[1, 2:4].cpu().tolist() == [[0, 0, 7, 7]] * 2 and (tab[0] == -7).all() and (tab[1, :2] == -7).all()
    assert eng.mask_boxes(m.view(torch.bool), record_out=False, hbox_out=False)[1].cpu().tolist() == [[[7, 0], [7, 7], [0, 7], [0, 0]]] * 2
    with pytest.raises(ValueError):
        eng.mask_boxes(m[0])
    with pytest.raises(ValueError):
        eng.mask_boxes(m, hbox_out=torch.zeros(2, 4, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        eng.mask_boxes(m, record_out=torch.zeros(3, 8, dtype=torch.int64, device="cuda"))
    with pytest.raises(AssertionError):
        eng.mask_boxes(m, offset=(32768, 0))


# ------------------------------------------------------------------------------------------------
# the option through the pipelines
# ------------------------------------------------------------------------------------------------
SIZES = [(1024, 1024), (600, 800)]
T = 16


def _items(driver):
    items = []
    for i, (h, w) in enumerate(SIZES):
        boxes, labels = synth.make_boxes(60 + i, 4, h, w)
        items.append(driver.WorkItem(f"B{i:04d}", synth.make_image(60 + i, h, w), boxes, labels))
    return items


def _collect(pipe, batches):
    got = {}

    def sink(results, release):
        for r in results:
            r.rles = [r.rle(j) for j in range(len(r.labels))] if r.rle_table is not None else None
            r.seg_mask = None if r.seg_mask is None else r.seg_mask.copy()
            r.masks = None if r.masks is None else r.masks.copy()
            r.rle_data = r.png_data = r.gt_rle_data = None
            got[r.key] = r
        release()

    pipe.run(batches, sink)
    return got


def _assert_result_boxes(eng, r, masks: np.ndarray, offset=(0, 0), what=""):
    """r.mask_hbox / mask_rbox / mask_record equal Engine.mask_boxes on `masks` and box_ref."""
    got = (r.mask_hbox, r.mask_rbox, r.mask_record)
    _assert_boxes(got, box_ref.mask_boxes(masks, *offset), what + " vs box_ref")
    if eng is not None:
        dev = eng.mask_boxes(torch.from_numpy(np.ascontiguousarray(masks)).cuda(), offset)
        _assert_boxes(got, tuple(t.cpu().numpy() for t in dev), what + " vs Engine.mask_boxes")


@pytest.mark.parametrize("min_region_area", [0, T])
def test_tile_pipeline_boxes_are_those_of_the_masks_that_go_out(min_region_area):
    from samrs_amd import driver
    sam = _sam(max_images=4, max_prompts=20, precision="f16")
    items = _items(driver)
    kw = dict(batch=2, box_batch=3, max_boxes=8, rle=True, rle_buffer_mb=64, keep_masks=True, min_region_area=min_region_area)
    on = _collect(driver.TilePipeline(sam, N_CLASSES, mask_boxes=True, **kw), driver.batched(items, 2))
    p0 = driver.TilePipeline(sam, N_CLASSES, **kw)
    off = _collect(p0, driver.batched(items, 2))
    assert not hasattr(p0, "hbox_dev")                               # off: nothing allocated
    for it in items:
        a, b = on[it.key], off[it.key]
        _assert_result_boxes(sam.engine, a, a.masks, what=it.key)
        for j in range(len(a.labels)):
            x0, y0, x1, y1 = (int(v) for v in a.mask_hbox[j])
            assert a.mask_bbox(j) == (None if a.mask_record[j, 6] == 0 else [x0, y0, x1 - x0 + 1, y1 - y0 + 1])
        assert b.mask_hbox is None and b.mask_rbox is None and b.mask_record is None
        for f in ("seg_mask", "areas", "masks", "rle_table", "changed"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f      # everything else is unchanged
        assert a.rles == b.rles


def test_instance_pipeline_boxes_of_the_kept_masks_and_of_the_ground_truth():
    from samrs_amd import driver
    sam = _sam(max_images=4, max_prompts=6)
    items = []
    for i, (h, w) in enumerate([(1024, 1024), (517, 803)]):
        polys, labels = synth.make_rboxes(90 + i, 4, h, w)
        cols = np.random.default_rng(90 + i).integers(0, 256, size=(4, 3), dtype=np.uint8)
        label = np.full((h, w, 3), 128, dtype=np.uint8)
        for j, p in enumerate(polys):
            x0, y0 = np.floor(p.min(0)).astype(int).clip(0)
            x1, y1 = np.ceil(p.max(0)).astype(int)
            label[y0:y1, x0:x1] = cols[j]
        items.append(driver.WorkItem(f"t{i}", synth.make_image(90 + i, h, w), polys, labels, (label, cols)))
    kw = dict(prompt="box", multimask=True, gt=True, batch=2, box_batch=3, max_boxes=8, rle=True, rle_buffer_mb=64, keep_masks=True)
    for t in (0, T):
        got = _collect(driver.InstancePipeline(sam, 1, mask_boxes=True, min_region_area=t, **kw), driver.batched(items, 2))
        for it in items:
            r = got[it.key]
            _assert_result_boxes(sam.engine, r, r.masks, what=f"{it.key} T={t}")
            label, cols = it.gt
            gt = (label[None] == cols[:, None, None, :]).all(-1).astype(np.uint8)
            assert np.array_equal(r.gt_hbox, box_ref.mask_boxes(gt)[0]), f"{it.key}: ground-truth hbox"
    off = _collect(driver.InstancePipeline(sam, 1, **kw), driver.batched(items, 2))
    assert all(r.mask_hbox is None and r.gt_hbox is None for r in off.values())


def test_scene_pipeline_boxes_are_in_the_scene_frame():
    from samrs_amd import driver, rle
    from samrs_amd.scene import ScenePipeline
    sam = _sam(max_images=8, max_prompts=64, precision="f16")
    H, W = 256, 448
    image = synth.make_image(33, H, W)
    boxes = np.array([[20, 30, 120, 200], [300, 40, 430, 180], [330, 100, 440, 250], [10, 10, 60, 60]], dtype=np.float32)
    labels = np.array([1, 2, 3, 4])
    for t in (0, T):
        pipe = ScenePipeline(sam, N_CLASSES, window=256, overlap=64, batch=2, box_batch=3, rle=True, rle_buffer_mb=16, mask_boxes=True,
                             min_region_area=t)
        r = _collect(pipe, [driver.WorkItem("scene", image, boxes, labels)])["scene"]
        assert len(r.windows) == 2 and sorted(set(r.window_of)) == [0, 1] and r.windows[1][0] > 0
        pasted = np.stack([rle.decode(d) for d in r.rles]).astype(np.uint8)      # each mask pasted at its window's offset
        assert pasted.shape == (4, H, W)
        _assert_result_boxes(None, r, pasted, what=f"scene T={t}")
        for j in range(4):                                           # and exactly the window-frame boxes shifted by the origin
            x0, y0, w, h = r.windows[r.window_of[j]]
            crop = np.ascontiguousarray(pasted[j, y0:y0 + h, x0:x0 + w])
            dev = sam.engine.mask_boxes(torch.from_numpy(crop[None]).cuda(), (x0, y0))
            _assert_boxes((r.mask_hbox[j:j + 1], r.mask_rbox[j:j + 1], r.mask_record[j:j + 1]), tuple(v.cpu().numpy() for v in dev),
                          f"scene box {j}")
    off = _collect(ScenePipeline(sam, N_CLASSES, window=256, overlap=64, rle=True, rle_buffer_mb=16),
                   [driver.WorkItem("scene", image, boxes, labels)])["scene"]
    assert off.mask_hbox is None and off.mask_rbox is None and off.mask_record is None


def test_generate_cli_pickle_entries_and_dota_files(tmp_path):
    from samrs_amd import driver, generate, rle, tile_io
    items = _items(driver)
    img_dir = tmp_path / "img"
    img_dir.mkdir()
    ann = {}
    for it in items:
        tile_io.write_rgb(str(img_dir / f"{it.key}.png"), it.image, 1)
        ann[it.key] = {"boxes": it.boxes.tolist(), "labels": it.labels.tolist()}
    (tmp_path / "boxes.json").write_text(json.dumps(ann))
    base = ["--images", str(img_dir), "--boxes", str(tmp_path / "boxes.json"), "--model", "vit_tiny", "--box-batch", "20", "--batch", "2"]
    generate.main(base + ["--out", str(tmp_path / "dota"), "--dota-txt"])
    generate.main(base + ["--out", str(tmp_path / "off")])
    names = [str(i) for i in range(N_CLASSES)]
    for it in items:
        with open(tmp_path / "dota" / "ins" / f"{it.key}.pkl", "rb") as f:
            info = pickle.load(f)
        with open(tmp_path / "off" / "ins" / f"{it.key}.pkl", "rb") as f:
            plain = pickle.load(f)
        masks = np.stack([rle.decode(e["mask"]) for e in info]).astype(np.uint8)
        hb, rb, rec = box_ref.mask_boxes(masks)
        lines = []
        for j, e in enumerate(info):
            if rec[j, 6] == 0:                                       # an empty mask: None twice, and no line
                assert e["mask_bbox"] is None and e["mask_rbox"] is None
                continue
            assert e["mask_bbox"] == [int(hb[j, 0]), int(hb[j, 1]), int(hb[j, 2] - hb[j, 0] + 1), int(hb[j, 3] - hb[j, 1] + 1)]
            assert e["mask_rbox"].dtype == np.float32 and e["mask_rbox"].tobytes() == rb[j].tobytes()
            lines.append(" ".join("%.1f" % v for v in rb[j].reshape(8)) + f" {names[e['label']]} {e['label']}")
        for e, q in zip(info, plain):                                # everything else is what a run without the flags writes
            stripped = {k: v for k, v in e.items() if k not in ("mask_bbox", "mask_rbox")}
            assert sorted(stripped) == sorted(q) and stripped["mask"] == q["mask"] and stripped["size"] == q["size"]
        assert open(tmp_path / "dota" / "rbox" / f"{it.key}.txt").read().splitlines() == lines
        for sub in ("gray", "color"):
            assert open(tmp_path / "dota" / sub / f"{it.key}.png", "rb").read() == open(tmp_path / "off" / sub / f"{it.key}.png", "rb").read()
    assert not (tmp_path / "off" / "rbox").exists()
    assert open(tmp_path / "dota" / "statistic" / "class_stats.json").read() == open(tmp_path / "off" / "statistic" / "class_stats.json").read()
