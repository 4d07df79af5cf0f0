"""GPU: samrs_clean_masks (region_kernels.hip: block-based union-find labelling, areas, small-region removal in place) and the
labelling alone (samrs_k_region_labels) against the host restatement tests/region_ref.py, then the option through both pipelines
and the generation CLI.  Integer work on both sides: every comparison is exact.

Shapes: the tile of the labelling kernels is 32 rows x 128 columns and a lane owns 16 pixels, so 67 x 93 (odd, one tile column),
70 x 272 (whole 16-pixel segments: the 16-byte path, three tile columns), 96 x 96, 130 x 130 and 1024 x 1024 cover both load
paths, partial tiles, several tile rows and columns and the full size."""
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
import region_ref  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("holes", "islands", "both")


def _sam(name="vit_tiny", **kw):
    import samrs_amd
    return samrs_amd.sam_model_registry[name](**kw).to("cuda")


@pytest.fixture(scope="module")
def eng():
    sam = _sam(max_images=1, max_prompts=4)
    yield sam.engine


def _run(eng, masks: np.ndarray, t: int, mode):
    """(cleaned masks, areas, changed) of the device on a copy of `masks`."""
    d = torch.from_numpy(np.ascontiguousarray(masks)).cuda()
    out, areas, changed = eng.clean_masks(d, t, mode)
    torch.cuda.synchronize()
    assert out.data_ptr() == d.data_ptr()                    # in place
    return d.cpu().numpy(), areas.cpu().numpy(), changed.cpu().numpy()


def _check(eng, masks: np.ndarray, t: int, mode, what=""):
    got, areas, changed = _run(eng, masks, t, mode)
    want, wa, wc = region_ref.clean_batch(masks, t, mode)
    assert got.max(initial=0) <= 1
    bad = [i for i in range(len(masks)) if not np.array_equal(got[i], want[i])]
    assert not bad, f"{what} T={t} {mode}: masks {bad} differ ({int((got != want).sum())} pixels)"
    assert np.array_equal(areas, wa), f"{what} T={t} {mode}: areas_out"
    assert np.array_equal(changed, wc), f"{what} T={t} {mode}: changed_out"
    return got, areas, changed


@pytest.mark.parametrize("shape", [(5, 67, 93), (3, 70, 272)])
@pytest.mark.parametrize("density", [0.3, 0.5, 0.7])
def test_random_masks_odd_and_segment_aligned_shapes(eng, shape, density):
    rng = np.random.default_rng(int(density * 100) + shape[2])
    masks = (rng.random(shape) < density).astype(np.uint8)
    for t in (1, 2, 5, 40, 10 ** 6):
        for mode in MODES:
            got, _, changed = _check(eng, masks, t, mode, f"{shape} p={density}")
            if t == 1:
                assert np.array_equal(got, masks) and not changed.any()
    for comp in (False, True):                               # the labelling alone
        lab = eng.region_labels(torch.from_numpy(masks).cuda(), complement=comp).cpu().numpy()
        for i in range(shape[0]):
            assert np.array_equal(lab[i], region_ref.labels(masks[i], comp)), f"labels of mask {i}, complement={comp}"


def _spiral(n: int) -> np.ndarray:
    """A one-pixel-wide spiral from (0, 0) inwards, one empty pixel between its arms."""
    m = np.zeros((n, n), dtype=np.uint8)
    y = x = d = 0
    m[0, 0] = 1
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))
    while True:
        for turn in (0, 1):
            dy, dx = dirs[(d + turn) % 4]
            ny, nx, fy, fx = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= fy < n and 0 <= fx < n and m[fy, fx]):
                y, x, d = ny, nx, (d + turn) % 4
                m[y, x] = 1
                break
        else:
            return m


def _serpentine(n: int) -> np.ndarray:
    m = np.zeros((n, n), dtype=np.uint8)
    m[0::2] = 1
    m[1::4, n - 1] = 1
    m[3::4, 0] = 1
    return m


@pytest.mark.parametrize("shape_fn", [_spiral, _serpentine])
def test_one_component_winding_through_every_tile(eng, shape_fn):
    m = shape_fn(96)
    length = int(m.sum())
    ref = region_ref.labels(m)
    assert length > 96 * 96 // 3 and set(ref[m == 1].tolist()) == {0}          # the construction: one component, first pixel (0, 0)
    lab = eng.region_labels(torch.from_numpy(m[None]).cuda()).cpu().numpy()[0]
    assert np.array_equal(lab, ref)
    assert np.array_equal(eng.region_labels(torch.from_numpy(m[None]).cuda(), complement=True).cpu().numpy()[0],
                          region_ref.labels(m, True))
    for t in (length, length + 1):                           # kept as it is; all small: kept as the largest
        got, areas, changed = _check(eng, m[None], t, "islands", shape_fn.__name__)
        assert np.array_equal(got[0], m) and areas[0] == length and changed[0] == 0
    for mode in ("holes", "both"):
        _check(eng, m[None], 50, mode, shape_fn.__name__)


def test_diagonals_across_tile_corners(eng):
    diag = np.eye(130, dtype=np.uint8)
    lab = eng.region_labels(torch.from_numpy(diag[None]).cuda()).cpu().numpy()[0]
    assert (lab[diag == 1] == 0).all() and (lab[diag == 0] == -1).all()
    anti = np.ascontiguousarray(diag[:, ::-1])               # root = (0, 129)
    lab = eng.region_labels(torch.from_numpy(anti[None]).cuda()).cpu().numpy()[0]
    assert (lab[anti == 1] == 129).all()
    for m in (diag, anti):
        got, areas, _ = _check(eng, m[None], 130, "islands", "diagonal")
        assert np.array_equal(got[0], m) and areas[0] == 130
        _check(eng, m[None], 131, "both", "diagonal")
    # a diagonal that crosses the corner where four tiles meet: rows 31 | 32, columns 127 | 128, in a 16-byte aligned image
    wide = np.zeros((64, 256), dtype=np.uint8)
    for k in range(-20, 20):
        wide[32 + k, 128 + k] = 1
    assert (eng.region_labels(torch.from_numpy(wide[None]).cuda()).cpu().numpy()[0][wide == 1] == 12 * 256 + 108).all()
    wide2 = np.ascontiguousarray(wide[:, ::-1])
    assert np.array_equal(eng.region_labels(torch.from_numpy(wide2[None]).cuda()).cpu().numpy()[0], region_ref.labels(wide2))
    yy, xx = np.mgrid[0:64, 0:64]
    board = ((yy + xx) % 2 == 0).astype(np.uint8)
    lab = eng.region_labels(torch.from_numpy(board[None]).cuda()).cpu().numpy()[0]
    assert (lab[board == 1] == 0).all()
    lab = eng.region_labels(torch.from_numpy(board[None]).cuda(), complement=True).cpu().numpy()[0]
    assert (lab[board == 0] == 1).all() and (lab[board == 1] == -1).all()
    for mode in MODES:
        got, _, changed = _check(eng, board[None], 2048, mode, "checkerboard")
        assert np.array_equal(got[0], board) and changed[0] == 0
    _check(eng, board[None], 2049, "both", "checkerboard")


def test_threshold_is_strict(eng):
    t = 6
    m = np.zeros((40, 150), dtype=np.uint8)
    m[2:7, 2:8] = 1
    m[3:5, 3:6] = 0                       # a ring with a hole of 6 = T pixels: stays open
    m[2:7, 120:132] = 1
    m[3:4, 124:129] = 0                   # a hole of 5 = T - 1 pixels across the tile border at column 128: filled
    m[20, 10:16] = 1                      # an island of T pixels: stays
    m[30:35, 127] = 1                     # an island of T - 1 pixels: goes
    got, _, _ = _check(eng, m[None], t, "both", "threshold")
    want = m.copy()
    want[3:4, 124:129] = 1
    want[30:35, 127] = 0
    assert np.array_equal(got[0], want)
    _check(eng, m[None], t, "holes", "threshold")
    _check(eng, m[None], t, "islands", "threshold")
    _check(eng, m[None], t + 1, "both", "threshold")


def test_tie_keeps_the_first_in_row_major_order(eng):
    m = np.zeros((70, 140), dtype=np.uint8)
    m[40, 126:129] = 1                    # 3 pixels across the tile border, first pixel (40, 126)
    m[40:43, 5] = 1                       # 3 pixels, first pixel (40, 5): comes first in row-major order
    m[10, 60:62] = 1                      # 2 pixels, earlier than both but smaller
    got, areas, changed = _check(eng, m[None], 10, "islands", "tie")
    want = np.zeros_like(m)
    want[40:43, 5] = 1
    assert np.array_equal(got[0], want) and areas[0] == 3 and changed[0] == 5


@pytest.mark.parametrize("shape", [(2, 50, 70), (2, 64, 256)])
def test_trivial_inputs(eng, shape):
    for mode in MODES:
        z = np.zeros(shape, dtype=np.uint8)
        got, areas, changed = _check(eng, z, 16, mode, "empty")
        assert not got.any() and not areas.any() and not changed.any()
        o = np.full(shape, 255, dtype=np.uint8)
        got, areas, changed = _check(eng, o, 16, mode, "full")
        assert (got == 1).all() and (areas == shape[1] * shape[2]).all() and not changed.any()
    rng = np.random.default_rng(5)
    m = ((rng.random(shape) < 0.6) * rng.integers(1, 256, size=shape)).astype(np.uint8)       # any non-zero byte is set
    for mode in MODES:
        _check(eng, m, 4, mode, "bytes")
    # bool tensors, and caller-owned output slices
    b = torch.from_numpy(m != 0).cuda()
    tab = torch.full((2, shape[0] + 2), -7, dtype=torch.int64, device="cuda")
    out, _, _ = eng.clean_masks(b, 4, "both", areas_out=tab[0, 1:-1], changed_out=tab[1, 1:-1])
    want, wa, wc = region_ref.clean_batch(m, 4, "both")
    assert out.dtype == torch.bool and np.array_equal(out.cpu().numpy(), want.astype(bool))
    th = tab.cpu().numpy()
    assert np.array_equal(th[0, 1:-1], wa) and np.array_equal(th[1, 1:-1], wc) and (th[:, 0] == -7).all() and (th[:, -1] == -7).all()


def test_masks_are_independent_and_chunked(eng):
    rng = np.random.default_rng(9)
    masks = (rng.random((70, 40, 40)) < rng.choice([0.2, 0.5, 0.8], size=(70, 1, 1))).astype(np.uint8)
    got, areas, changed = _check(eng, masks, 7, "both", "70 masks")
    for i in (0, 31, 32, 63, 64, 69):                        # each mask alone, on the device too
        g1, a1, c1 = _run(eng, masks[i:i + 1], 7, "both")
        assert np.array_equal(g1[0], got[i]) and a1[0] == areas[i] and c1[0] == changed[i]


def test_full_size_blob_with_speckle(eng):
    masks = np.stack([region_ref.speckled_ellipse(100 + i) for i in range(3)])
    got, areas, changed = _check(eng, masks, 16, "both", "1024^2")
    assert (changed > 0).all()
    for i in range(3):
        assert len(np.unique(region_ref.labels(got[i]))) == 2               # one component and the background


def test_bad_arguments(eng):
    from samrs_amd import engine
    m = torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda")
    a = torch.zeros(1, dtype=torch.int64, device="cuda")
    lib, h = eng.lib, eng.handle
    assert lib.samrs_clean_masks(h, m.data_ptr(), 1, 8, 8, 0, 3, a.data_ptr(), a.data_ptr(), None) == engine.ERR_BAD_ARG
    assert lib.samrs_clean_masks(h, m.data_ptr(), 1, 8, 8, 4, 0, a.data_ptr(), a.data_ptr(), None) == engine.ERR_BAD_ARG
    assert lib.samrs_clean_masks(h, m.data_ptr(), 1, 8, 8, 4, 4, a.data_ptr(), a.data_ptr(), None) == engine.ERR_BAD_ARG
    assert lib.samrs_clean_masks(h, m.data_ptr(), 0, 8, 8, 4, 3, a.data_ptr(), a.data_ptr(), None) == engine.ERR_BAD_ARG
    assert lib.samrs_clean_masks(h, None, 1, 8, 8, 4, 3, a.data_ptr(), a.data_ptr(), None) == engine.ERR_BAD_ARG
    assert lib.samrs_clean_masks(h, m.data_ptr(), 1, 1 << 15, 1 << 15, 4, 3, None, None, None) == engine.ERR_BAD_ARG
    assert lib.samrs_clean_masks(h, m.data_ptr(), 1, 8, 8, 4, 3, None, None, None) == engine.OK       # both outputs may be NULL
    with pytest.raises(ValueError):
        eng.clean_masks(m, 4, "speckle")
    with pytest.raises(ValueError):
        eng.clean_masks(m[0], 4)
    with pytest.raises(AssertionError):
        eng.clean_masks(m, 0)
    with pytest.raises(ValueError):
        eng.clean_masks(m, 4, areas_out=torch.zeros(3, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        eng.clean_masks(m, 4, changed_out=torch.zeros(1, dtype=torch.int32, device="cuda"))
    _, areas, changed = eng.clean_masks(m, 4, areas_out=False)              # an output nobody asked for is not computed
    assert areas is None and int(changed[0]) == 0
    assert eng.clean_masks(m, 4, areas_out=False, changed_out=False)[1:] == (None, None)


# ------------------------------------------------------------------------------------------------
# the option through the pipelines
# ------------------------------------------------------------------------------------------------
T = 16
SIZES = [(1024, 1024), (1024, 1024), (600, 800)]
N_CLASSES = 18


def _items(driver):
    items = []
    for i, (h, w) in enumerate(SIZES):
        boxes, labels = synth.make_boxes(80 + i, 5, h, w)
        items.append(driver.WorkItem(f"P{i:04d}", synth.make_image(80 + i, h, w), boxes, labels))
    return items


def _device_rles(eng, masks: torch.Tensor):
    n, h, w = masks.shape
    out = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    cur = torch.zeros(1, dtype=torch.int64, device="cuda")
    tab = torch.zeros(n, 3, dtype=torch.int64, device="cuda")
    eng.rle_encode(masks, out, cur, tab)
    data, tab = out[:int(cur.item())].cpu().numpy(), tab.cpu().numpy()
    assert (tab[:, 1] >= 0).all()
    return [{"size": [h, w], "counts": data[o:o + l].tobytes().decode("ascii")} for o, l, _ in tab]


@functools.lru_cache(maxsize=None)
def _serial_reference():
    """Per tile (class map, areas, cleaned masks, RLE dicts, changed) and the class statistics of the serial composition of entry
    points that have their own tests: Engine.predict -> region_ref on the host -> Engine.paint / Engine.rle_encode on the uploaded
    cleaned masks.  Computed once for all the pipeline tests."""
    import samrs_amd
    from samrs_amd import driver
    sam = _sam(max_images=4, max_prompts=20, precision="f16")
    eng, pred = sam.engine, samrs_amd.SamPredictor(sam)
    cpix = torch.zeros(N_CLASSES, dtype=torch.int64, device="cuda")
    cins = torch.zeros(N_CLASSES, dtype=torch.int64, device="cuda")
    per = {}
    # the operand-split mode the pipelines' own calls run in (their precision="auto"), whatever the engine's default is
    split = driver.TilePipeline._choose_split(sam, "auto", multimask=False)
    for it in _items(driver):
        h, w = it.image.shape[:2]
        with eng.options(**({} if split is None else {"split": split})):
            pred.set_image(it.image)
            tb = pred.transform.apply_boxes_torch(torch.from_numpy(it.boxes).cuda(), (h, w))
            masks, _, _ = pred.predict_torch(None, None, tb, None, multimask_output=False)
        cleaned, areas, changed = region_ref.clean_batch(masks[:, 0].cpu().numpy(), T, "both")
        dev = torch.from_numpy(cleaned).cuda()
        seg = torch.full((h, w), 255, dtype=torch.uint8, device="cuda")
        a = eng.paint(dev, torch.from_numpy(it.labels.astype(np.int32)).cuda(), seg, cpix, cins)
        assert np.array_equal(a.cpu().numpy(), areas)
        per[it.key] = (seg.cpu().numpy(), areas, cleaned, _device_rles(eng, dev), changed)
    return per, cpix.cpu().numpy(), cins.cpu().numpy()


def _collect(pipe, items, batch=2):
    from samrs_amd import driver
    got = {}

    def sink(results, release):
        for r in results:
            r.rles = [r.rle(j) for j in range(len(r.labels))] if r.rle_table is not None else None
            r.pngs = (bytes(r.png("gray")), bytes(r.png("color"))) if r.png_table is not None else None
            r.seg_mask = None if r.seg_mask is None else r.seg_mask.copy()
            r.masks = None if r.masks is None else r.masks.copy()
            r.rle_table = None if r.rle_table is None else r.rle_table.copy()
            r.rle_data = r.png_data = r.gt_rle_data = None
            got[r.key] = r
        release()

    assert pipe.run(driver.batched(items, batch), sink) == len(items)
    return got


@pytest.mark.parametrize("variant", ["plain", "batch_decode", "png_lut"])
def test_tile_pipeline_cleans_before_anything_reads_the_masks(variant, tmp_path):
    from samrs_amd import driver, generate, tile_io
    per, cpix, cins = _serial_reference()
    sam = _sam(max_images=4, max_prompts=20, precision="f16")
    items = _items(driver)
    kw = {}
    if variant == "batch_decode":
        kw["batch_decode"] = True
    if variant == "png_lut":
        kw["png_lut"] = tile_io.class_lut(generate.default_palette(N_CLASSES))
    pipe = driver.TilePipeline(sam, N_CLASSES, batch=2, box_batch=3, max_boxes=8, rle=True, rle_buffer_mb=64, keep_masks=True,
                               min_region_area=T, **kw)
    got = _collect(pipe, items)
    total = 0
    for it in items:
        r = got[it.key]
        seg, areas, cleaned, rles, changed = per[it.key]
        assert np.array_equal(r.masks, cleaned), f"{it.key}: kept masks"
        assert np.array_equal(r.seg_mask, seg), f"{it.key}: class map"
        assert np.array_equal(r.areas, areas) and np.array_equal(r.changed, changed)
        assert r.rles == rles, f"{it.key}: RLE strings"
        total += int(r.changed.sum())
        if variant == "png_lut":
            g, c = str(tmp_path / "g.png"), str(tmp_path / "c.png")
            tile_io.write_label_pair(g, c, seg, kw["png_lut"])
            assert r.pngs == (open(g, "rb").read(), open(c, "rb").read()), f"{it.key}: device PNG files"
    assert total > 0                                          # random-init weights paint noise-like masks: there is speckle to remove
    assert np.array_equal(pipe.class_pixels.cpu().numpy(), cpix) and np.array_equal(pipe.class_instances.cpu().numpy(), cins)


def test_option_off_changes_nothing():
    from samrs_amd import driver
    sam = _sam(max_images=4, max_prompts=20, precision="f16")
    items = _items(driver)
    kw = dict(batch=2, box_batch=3, max_boxes=8, rle=True, rle_buffer_mb=64, keep_masks=True)
    a = _collect(driver.TilePipeline(sam, N_CLASSES, **kw), items)
    p0 = driver.TilePipeline(sam, N_CLASSES, min_region_area=0, region_mode="islands", **kw)
    b = _collect(p0, items)
    assert not hasattr(p0, "chg_dev")
    for it in items:
        ra, rb = a[it.key], b[it.key]
        assert rb.changed is None and ra.changed is None
        for f in ("seg_mask", "areas", "boxes", "labels", "masks", "rle_table"):
            assert np.array_equal(getattr(ra, f), getattr(rb, f)), f
        assert ra.rles == rb.rles and ra.size == rb.size and ra.quality is None and rb.quality is None
        assert ra.inter is None and rb.inter is None and ra.png_table is None and rb.png_table is None
    with pytest.raises(ValueError):
        driver.TilePipeline(sam, N_CLASSES, min_region_area=4, region_mode="speckle", **kw)
    with pytest.raises(ValueError):
        driver.TilePipeline(sam, N_CLASSES, min_region_area=-1, **kw)


@pytest.mark.parametrize("multimask", [True, False])
def test_instance_pipeline_tables_hold_the_cleaned_masks(multimask):
    from samrs_amd import driver, rle
    sam = _sam(max_images=4, max_prompts=6)
    items = []
    for i, (h, w) in enumerate([(1024, 1024), (517, 803)]):
        polys, labels = synth.make_rboxes(90 + i, 5, h, w)
        cols = np.random.default_rng(90 + i).integers(0, 256, size=(5, 3), dtype=np.uint8)
        label = np.full((h, w, 3), 128, dtype=np.uint8)
        for j, p in enumerate(polys):                        # ground truth: each object's enclosing box in its colour
            x0, y0 = np.floor(p.min(0)).astype(int).clip(0)
            x1, y1 = np.ceil(p.max(0)).astype(int)
            label[y0:y1, x0:x1] = cols[j]
        items.append(driver.WorkItem(f"t{i}", synth.make_image(90 + i, h, w), polys, labels, (label, cols)))
    kw = dict(prompt="box", multimask=multimask, gt=True, batch=2, box_batch=3, max_boxes=8, rle=True, rle_buffer_mb=64, keep_masks=True)

    def collect(pipe):
        got = {}

        def sink(results, release):
            for r in results:
                r.rles = [r.rle(j) for j in range(len(r.labels))]
                r.gts = [r.gt_rle(j) for j in range(len(r.labels))]
                r.masks = r.masks.copy()
                got[r.key] = r
            release()

        assert pipe.run(driver.batched(items, 2), sink) == len(items)
        return got

    off = collect(driver.InstancePipeline(sam, 1, **kw))
    on = collect(driver.InstancePipeline(sam, 1, min_region_area=T, **kw))
    total = 0
    for it in items:
        a, b = on[it.key], off[it.key]
        cleaned, areas, changed = region_ref.clean_batch(b.masks, T, "both")
        label, cols = it.gt
        gt = (label[None] == cols[:, None, None, :]).all(-1)
        assert b.changed is None
        assert np.array_equal(a.masks, cleaned), it.key
        assert np.array_equal(a.areas, areas) and np.array_equal(a.changed, changed)
        assert np.array_equal(a.inter, (cleaned.astype(bool) & gt).reshape(len(cols), -1).sum(1))
        assert np.array_equal(a.gt_area, b.gt_area) and np.array_equal(a.quality, b.quality)
        for j in range(len(cols)):
            assert a.rles[j] == rle.encode(cleaned[j].astype(bool)), f"{it.key} object {j}"
        assert a.gts == b.gts
        total += int(changed.sum())
    assert total > 0


def test_generate_cli_writes_the_cleaned_labels(tmp_path):
    from PIL import Image
    from samrs_amd import driver, generate, tile_io
    per, _, _ = _serial_reference()
    items = _items(driver)[:2]
    img_dir = tmp_path / "img"
    img_dir.mkdir()
    ann = {}
    for it in items:
        tile_io.write_rgb(str(img_dir / f"{it.key}.png"), it.image, 1)
        ann[it.key] = {"boxes": it.boxes.tolist(), "labels": it.labels.tolist()}
    (tmp_path / "boxes.json").write_text(json.dumps(ann))
    out = tmp_path / "out"
    generate.main(["--images", str(img_dir), "--boxes", str(tmp_path / "boxes.json"), "--out", str(out), "--model", "vit_tiny",
                   "--box-batch", "20", "--batch", "2", "--min-region-area", str(T)])
    for it in items:
        seg, areas, _, rles, _ = per[it.key]
        assert np.array_equal(np.array(Image.open(out / "gray" / f"{it.key}.png")), seg), it.key
        with open(out / "ins" / f"{it.key}.pkl", "rb") as f:
            info = pickle.load(f)
        assert [e["size"] for e in info] == areas.tolist()
        assert [e["mask"] for e in info] == rles
    stats = json.load(open(out / "statistic" / "class_stats.json"))
    changed = np.concatenate([per[it.key][4] for it in items])
    assert stats["region_cleanup"] == {"min_region_area": T, "region_mode": "both", "changed_pixel_num": int(changed.sum()),
                                       "changed_instance_num": int((changed > 0).sum())}
    # without the flag the statistics file has the keys it always had
    off = tmp_path / "off"
    generate.main(["--images", str(img_dir), "--boxes", str(tmp_path / "boxes.json"), "--out", str(off), "--model", "vit_tiny",
                   "--box-batch", "20", "--batch", "2"])
    assert sorted(json.load(open(off / "statistic" / "class_stats.json"))) == ["class_instance_num", "class_pixel_num", "mask_num"]
