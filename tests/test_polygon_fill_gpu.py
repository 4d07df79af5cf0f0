"""GPU: samrs_fill_polygons (polygon_fill_kernels.hip: one workgroup per row and band of mask rows, toggle bits in LDS, prefix parity,
bytes out and `ref` in) against the host statements -- tests/polygon_fill_ref.py for the small cases, polygons.rasterize_any (pinned to
it in tests/test_polygon_fill_host.py) for the larger ones: every byte and all three counts, exactly.  Then the `polygon_iou` option
through the tile pipeline, generate and relabel, and relabel --masks-from polygons.

Shapes: 1 x 1, 1 x 70, 70 x 1 (one word, one row, one column), 70 x 99 (two bands of 64 rows; rows that begin at no multiple of 16:
the bytewise path), 64 x 64 (16-byte path, two words per row), 65 x 129 (a last band of one row, a last word of one column); 4 x 401
(200 toggles on the same words), 701 x 40 (an edge through eleven bands), 3 x 8192 (the carry through 256 words and four ballots; a
band of 32 rows), 1024 x 1024 with three rows (the production shape)."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from samrs_amd import polygons, rle, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polygon_fill_ref as pf_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N_CLASSES = 18
GUARD, SENTINEL = 80, 0xA5         # bytes on both sides of the mask buffer; 80 keeps the 16-byte alignment of the first mask
ALL_EDGES = 1 << 21


def _sam(name="vit_tiny", **kw):
    import samrs_amd
    return samrs_amd.sam_model_registry[name](**kw).to("cuda")


@pytest.fixture(scope="module")
def eng():
    sam = _sam(max_images=1, max_prompts=4)
    yield sam.engine


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _guarded(n, h, w):
    """(the flat buffer, its [n, h, w] view, the flat counts buffer, its [n, 3] view): sentinels on both sides of each"""
    buf = torch.full((2 * GUARD + n * h * w,), SENTINEL, dtype=torch.uint8, device="cuda")
    cnt = torch.full((n * 3 + 4,), -77, dtype=torch.int64, device="cuda")
    return buf, buf[GUARD:GUARD + n * h * w].view(n, h, w), cnt, cnt[2:2 + n * 3].view(n, 3)


def _guards_intact(buf, cnt, what):
    b, c = buf.cpu().numpy(), cnt.cpu().numpy()
    assert (b[:GUARD] == SENTINEL).all() and (b[-GUARD:] == SENTINEL).all(), f"{what}: a store outside the masks"
    assert (c[:2] == -77).all() and (c[-2:] == -77).all(), f"{what}: a store outside the counts"


def _fill_checked(eng, table, rings, vertices, h, w, origin, ref, want, is_rings, what):
    """one call into guarded buffers: masks == want, counts == the recount of want against ref"""
    n = int(table.shape[0])
    buf, out, cnt, counts = _guarded(n, h, w)
    got_m, got_c = eng.fill_polygons(table, rings, vertices, (h, w), origin, out=out, ref=ref, counts_out=counts)
    torch.cuda.synchronize()
    assert got_m.data_ptr() == out.data_ptr() and got_c.data_ptr() == counts.data_ptr()
    m, c = out.cpu().numpy(), counts.cpu().numpy()
    g = None if ref is None else ref.cpu().numpy()
    for j in range(n):
        assert np.array_equal(m[j], want[j]), f"{what} row {j}: {int((m[j] != want[j]).sum())} pixels differ"
        assert c[j].tolist() == pf_ref.counts(want[j], None if g is None else g[j], is_rings[j]), f"{what} row {j}: counts"
    _guards_intact(buf, cnt, what)
    return m, c


def _fill_lists(eng, lists, h, w, origin=(0, 0), ref=None, want=None, what=""):
    t, r, v = _dev(*polygons.pack_rings(lists))
    if want is None:
        want = [pf_ref.fill(rl, h, w, origin) for rl in lists]
    is_rings = [pf_ref.placed(rl, *origin) for rl in lists]
    return _fill_checked(eng, t, r, v, h, w, origin, ref, want, is_rings, what)


# ------------------------------------------------------------------------------------------------
# masks -> rings -> masks
# ------------------------------------------------------------------------------------------------
def _masks(h, w, seed):
    """speckle; a blob with holes and islands inside the holes; everything set"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.maximum(np.abs(yy - h / 2 + 0.5) / max(h / 2, 1), np.abs(xx - w / 2 + 0.5) / max(w / 2, 1))
    nested = ((d < 0.9) & ~((d < 0.7) & ~((d < 0.5) & ~(d < 0.25)))).astype(np.uint8)
    return np.stack([(rng.random((h, w)) < 0.45).astype(np.uint8), nested, np.ones((h, w), np.uint8)])


ROUND_TRIP_SIZES = [(1, 1), (1, 70), (70, 1), (70, 99), (64, 64), (65, 129)]


@pytest.mark.parametrize("h,w", ROUND_TRIP_SIZES)
def test_fill_inverts_the_tracing(eng, h, w):
    masks = _masks(h, w, 7 * h + w)
    d, = _dev(masks)
    v, r, _, t = eng.mask_polygons(d, (0, 0), ALL_EDGES)
    assert (t[:, 1] >= 0).all()
    m, c = _fill_checked(eng, t, r, v, h, w, (0, 0), d, masks, [True] * 3, f"{h} x {w}")
    area = masks.reshape(3, -1).sum(1)
    assert c.tolist() == [[int(a)] * 3 for a in area]
    # the same rings traced in a window at (40, 1000): the origin is subtracted again
    v, r, _, t = eng.mask_polygons(d, (40, 1000), ALL_EDGES)
    _fill_checked(eng, t, r, v, h, w, (40, 1000), d, masks, [True] * 3, f"{h} x {w} at (40, 1000)")


@pytest.mark.parametrize("eps", [0.5, 2.0, 8.0])
def test_fill_of_simplified_rings_is_rasterize_any(eng, eps):
    changed = 0
    for h, w in ROUND_TRIP_SIZES:
        masks = _masks(h, w, 3 * h + w)
        d, = _dev(masks)
        v, r, c, t = eng.mask_polygons(d, (0, 0), ALL_EDGES)
        eng.simplify_polygons(t, r, v, c, eps)
        tn, rn, vn = (x.cpu().numpy() for x in (t, r, v))
        lists = [polygons.rings_of(tn, rn, vn, j) for j in range(3)]
        want = [polygons.rasterize_any(rl, h, w) for rl in lists]
        changed += sum(int((want[j] != masks[j]).sum()) for j in range(3))
        _fill_checked(eng, t, r, v, h, w, (0, 0), d, want, [True] * 3, f"{h} x {w} eps {eps}")
    assert changed > 0 or eps < 1, "nothing was simplified"


# ------------------------------------------------------------------------------------------------
# hand-built rings
# ------------------------------------------------------------------------------------------------
def _comb(teeth=200):
    """a bar in row 3 with `teeth` one-pixel teeth in rows 1 .. 2, as one ring: every tooth's two vertical edges toggle rows 1 and 2"""
    pts = [(0, 3)]
    for i in range(teeth):
        pts += [(2 * i, 1), (2 * i + 1, 1), (2 * i + 1, 3)] if i == 0 else [(2 * i, 3), (2 * i, 1), (2 * i + 1, 1), (2 * i + 1, 3)]
    pts += [(2 * teeth + 1, 3), (2 * teeth + 1, 4), (0, 4)]
    return np.array(pts)


HAND = {
    "tie triangle": ([np.array([[0, 0], [8, 8], [0, 8]])], 8, 8, (0, 0)),
    "bow-tie": ([np.array([[1, 1], [9, 9], [9, 1], [1, 9]])], 10, 10, (0, 0)),
    "two overlapping rings": ([np.array([[1, 1], [20, 2], [18, 12], [2, 11]]), np.array([[10, 5], [30, 6], [28, 15], [9, 14]])], 17, 33, (0, 0)),
    "outside the window": ([np.array([[100, 100], [120, 100], [110, 130]])], 20, 20, (0, 0)),
    "far larger than the window": ([np.array([[-5000, -4000], [6000, -4500], [7000, 5000], [-6500, 6000]])], 21, 35, (0, 0)),
    "negative and beyond, origin (37, 11)": ([np.array([[-30, -20], [90, 5], [140, 60], [60, 95], [-10, 40]]),
                                              np.array([[50, 20], [70, 30], [45, 50]])], 45, 50, (37, 11)),
    "comb of 200 teeth": ([_comb()], 4, 401, (0, 0)),
    "an edge over 700 rows": ([np.array([[2, 0], [38, 700], [3, 700]])], 701, 40, (0, 0)),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_built_rings(eng, name):
    rings, h, w, origin = HAND[name]
    rl = [(p, False) for p in rings]
    want = pf_ref.fill(rl, h, w, origin)
    assert np.array_equal(polygons.rasterize_any(rl, h, w, origin), want)
    if name == "outside the window":
        assert not want.any()
    elif name == "far larger than the window":
        assert want.all()
    elif name == "comb of 200 teeth":
        assert want[1].sum() == 200 and want[3].sum() == 401 and not want[0].any()
    else:
        assert want.any() and not want.all()
    rng = np.random.default_rng(len(name))
    ref, = _dev((rng.random((1, h, w)) < 0.5).astype(np.uint8))
    _fill_lists(eng, [rl], h, w, origin, ref=ref, want=[want], what=name)


def test_width_carry_and_the_production_shape(eng):
    h, w = 3, 8192
    lists = [[(np.array([[5, 0], [8190, 0], [8190, 3], [5, 3]]), False)],
             [(np.array([[5, 0], [8190, 1], [8000, 3], [40, 2]]), False), (np.array([[100, 0], [4000, 0], [4100, 3], [90, 3]]), True)]]
    want = [polygons.rasterize_any(rl, h, w) for rl in lists]
    assert want[0][:, 5:8190].all() and not want[0][:, :5].any() and not want[0][:, 8190:].any()
    rng = np.random.default_rng(5)
    ref, = _dev((rng.random((2, h, w)) < 0.5).astype(np.uint8))
    _fill_lists(eng, lists, h, w, ref=ref, want=want, what="3 x 8192")
    h = w = 1024
    lists = []
    for j in range(3):
        ang = np.sort(rng.uniform(0, 2 * np.pi, 40))
        rad = rng.uniform(150, 520, 40)
        outer = np.stack([512 + rad * np.cos(ang), 500 + rad * np.sin(ang)], 1).round().astype(np.int64)
        lists.append([(outer, False), (np.array([[450, 450], [560, 470], [540, 560], [460, 540]]) + 10 * j, True)])
    want = [polygons.rasterize_any(rl, h, w) for rl in lists]
    ref, = _dev(np.stack([np.roll(m, 9, axis=1) for m in want]))
    m, c = _fill_lists(eng, lists, h, w, ref=ref, want=want, what="1024 x 1024")
    assert (c[:, 2] < c[:, 0]).all() and (c[:, 2] > 0).all()


# ------------------------------------------------------------------------------------------------
# rows that are not rings; null outputs; errors
# ------------------------------------------------------------------------------------------------
def test_rows_that_are_not_rings(eng):
    h, w = 40, 52
    tri = (np.array([[3, 2], [48, 9], [20, 37]]), False)
    quad = (np.array([[10, 10], [30, 10], [30, 30], [10, 30]]), False)
    far = (np.array([[0, 0], [(1 << 20) + 1, 0], [0, 30]]), False)
    near = (np.array([[0, 0], [1 << 20, 0], [0, 30]]), False)
    lists = [[tri], None, [quad, tri], [], [far], [near], [quad], [tri, quad], [quad], None, [tri]]
    t, r, v = polygons.pack_rings(lists)
    t[1] = (-1, -3, -1, -13, 12)                                    # not placed: what a full buffer leaves
    r[int(t[6, 0]), 0] = 1                                          # row 6: its ring does not begin at the row's first vertex
    r[int(t[7, 0]) + 1, 1] -= 1                                     # row 7: its rings end one short of the row's vertices
    t[8, 3] = 0                                                     # row 8: rings without vertices
    want = [pf_ref.fill(rl, h, w) for rl in lists]
    assert t[9].tolist() == [-1, -1, -1, -1, 0]                     # row 9: not traced, between real rows, as pack_rings writes it
    is_rings = [True, False, True, True, False, True, False, False, False, False, True]
    for j in (1, 4, 6, 7, 8, 9):
        want[j] = np.zeros((h, w), np.uint8)
    assert want[5].any()
    rng = np.random.default_rng(1)
    ref, = _dev((rng.random((len(lists), h, w)) < 0.5).astype(np.uint8))
    td, rd, vd = _dev(t, r, v)
    m, c = _fill_checked(eng, td, rd, vd, h, w, (0, 0), ref, want, is_rings, "mixed rows")
    assert c[1].tolist() == [-1, int(ref[1].sum()), 0] and c[9].tolist() == [-1, int(ref[9].sum()), 0]
    assert c[3].tolist() == [0, int(ref[3].sum()), 0] and np.array_equal(m[10], m[0]) and c[10, 0] == c[0, 0] > 0
    # ref NULL: the last two counts are 0; masks_out NULL: the same counts, and nothing else to write
    _fill_checked(eng, td, rd, vd, h, w, (0, 0), None, want, is_rings, "no ref")
    none, only = eng.fill_polygons(td, rd, vd, (h, w), out=False, ref=ref)
    assert none is None and np.array_equal(only.cpu().numpy(), c)
    masks, no_counts = eng.fill_polygons(td, rd, vd, (h, w))
    assert no_counts is None and np.array_equal(masks.cpu().numpy(), m)
    assert np.array_equal(polygons.fill_device(eng, lists[:4], h, w).cpu().numpy(), m[:4])


def test_no_rows_null_outputs_and_bad_arguments(eng):
    from samrs_amd import engine
    h, w = 12, 20
    t, r, v = _dev(*polygons.pack_rings([[np.array([[1, 1], [15, 2], [7, 10]])]]))
    buf, out, cnt, counts = _guarded(1, h, w)
    ref = torch.ones(1, h, w, dtype=torch.uint8, device="cuda")

    def call(vp, rp, tp, n, hh, ww, x0, y0, mp, gp, cp):
        return eng.lib.samrs_fill_polygons(eng.handle, vp, rp, tp, n, hh, ww, x0, y0, mp, gp, cp, None)

    V, R, T, M, G, C = (x.data_ptr() for x in (v, r, t, out, ref, counts))
    assert call(V, R, T, 0, h, w, 0, 0, M, G, C) == engine.OK       # no rows: nothing happens
    for args in ((V, R, T, 1, h, w, 0, 0, None, G, None),           # both outputs null
                 (V, R, T, -1, h, w, 0, 0, M, G, C), (None, R, T, 1, h, w, 0, 0, M, G, C), (V, None, T, 1, h, w, 0, 0, M, G, C),
                 (V, R, None, 1, h, w, 0, 0, M, G, C), (V, R, T, 1, 0, w, 0, 0, M, G, C), (V, R, T, 1, h, 8193, 0, 0, M, G, C),
                 (V, R, T, 1, h, w, -1, 0, M, G, C), (V, R, T, 1, h, w, 0, 32768, M, G, C)):
        assert call(*args) == engine.ERR_BAD_ARG, args
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all() and (cnt == -77).all()           # nothing was written by any of them
    with pytest.raises(AssertionError):
        eng.fill_polygons(t, r, v, (h, w), out=False, counts_out=False)
    empty = torch.zeros(0, 5, dtype=torch.int64, device="cuda")
    m0, c0 = eng.fill_polygons(empty, r, v, (h, w), ref=torch.zeros(0, h, w, dtype=torch.uint8, device="cuda"))
    assert tuple(m0.shape) == (0, h, w) and tuple(c0.shape) == (0, 3)
    assert call(V, R, T, 1, h, w, 0, 0, M, G, C) == engine.OK       # and the buffers do work
    torch.cuda.synchronize()
    assert out.sum().item() == counts[0, 0].item() == counts[0, 2].item() > 0 and counts[0, 1].item() == h * w


# ------------------------------------------------------------------------------------------------
# the option through the pipeline and the CLIs
# ------------------------------------------------------------------------------------------------
SIZES = [(256, 320), (192, 256)]
EPS = 1.0


def _items(driver):
    items = []
    for i, (h, w) in enumerate(SIZES):
        boxes, labels = synth.make_boxes(60 + i, 3, h, w)
        items.append(driver.WorkItem(f"B{i:04d}", synth.make_image(60 + i, h, w), boxes, labels))
    return items


def _collect(pipe, batches):
    got = {}

    def sink(results, release):
        for r in results:
            n = len(r.labels)
            got[r.key] = dict(rles=[r.rle(j) for j in range(n)], polys=[r.polygons(j) for j in range(n)], table=r.polygon_table.copy(),
                              rings=r.polygon_rings.copy(), vertices=r.polygon_vertices.copy(), areas=r.areas.copy(), seg=r.seg_mask.copy(),
                              counts=None if r.polygon_counts is None else r.polygon_counts.copy(),
                              ious=None if r.polygon_counts is None else [r.polygon_iou(j) for j in range(n)])
        release()

    pipe.run(batches, sink)
    return got


@pytest.mark.parametrize("batch_decode", [False, True])
def test_tile_pipeline_counts_what_the_tolerance_costs_and_changes_nothing(batch_decode):
    from samrs_amd import driver
    sam = _sam(max_images=4, max_prompts=20, precision="f16")
    items = _items(driver)
    kw = dict(batch=2, box_batch=2, max_boxes=8, rle=True, rle_buffer_mb=16, batch_decode=batch_decode, polygons=True, polygon_buffer_mb=16,
              polygon_max_edges=ALL_EDGES)
    on = _collect(driver.TilePipeline(sam, N_CLASSES, polygon_epsilon=EPS, polygon_iou=True, **kw), driver.batched(items, 2))
    off = _collect(driver.TilePipeline(sam, N_CLASSES, polygon_epsilon=EPS, **kw), driver.batched(items, 2))
    lossy = 0
    for it in items:
        a, b = on[it.key], off[it.key]
        assert b["counts"] is None and a["counts"].shape == (len(it.labels), 3)
        for f in ("table", "rings", "vertices", "areas", "seg"):   # box_batch 2 of 3 boxes: chunk by chunk equals the batch at once
            assert np.array_equal(a[f], b[f]), f"{it.key}: {f}"
        assert a["rles"] == b["rles"]
        h, w = it.image.shape[:2]
        for j in range(len(it.labels)):
            mask = rle.decode(a["rles"][j])
            fill = polygons.rasterize_any(a["polys"][j], h, w)
            assert a["counts"][j].tolist() == pf_ref.counts(fill, mask), f"{it.key} instance {j}"
            assert a["ious"][j] == float(polygons.iou_from_counts(a["counts"][j]))
            lossy += int(a["counts"][j, 2] != a["counts"][j, 1])
    assert lossy > 0, "the tolerance cost nothing: the test shows nothing"
    zero = _collect(driver.TilePipeline(sam, N_CLASSES, polygon_epsilon=0.0, polygon_iou=True, **kw), driver.batched(items, 2))
    for it in items:
        z = zero[it.key]
        assert (z["table"][:, 1] >= 0).all()
        assert z["counts"].tolist() == [[int(a)] * 3 for a in z["areas"]] and z["ious"] == [1.0] * len(it.labels)


def _load(root, sub, key):
    with open(os.path.join(root, sub, "ins", f"{key}.pkl"), "rb") as f:
        return pickle.load(f)


def _read(root, sub, kind, key):
    with open(os.path.join(root, sub, kind, f"{key}.png"), "rb") as f:
        return f.read()


def test_generate_reports_the_iou_and_relabel_rebuilds_from_polygons(tmp_path):
    from PIL import Image
    from samrs_amd import driver, generate, relabel, tile_io
    items = _items(driver)
    root = str(tmp_path)
    os.mkdir(os.path.join(root, "img"))
    ann = {}
    for it in items:
        tile_io.write_rgb(os.path.join(root, "img", f"{it.key}.png"), it.image, 1)
        ann[it.key] = {"boxes": it.boxes.tolist(), "labels": it.labels.tolist()}
    with open(os.path.join(root, "boxes.json"), "w") as f:
        json.dump(ann, f)
    base = ["--images", os.path.join(root, "img"), "--boxes", os.path.join(root, "boxes.json"), "--model", "vit_tiny", "--box-batch", "20",
            "--batch", "2", "--polygon-buffer-mb", "16", "--polygon-max-edges", str(ALL_EDGES)]
    poly = ["--n-classes", str(N_CLASSES), "--polygon-buffer-mb", "16", "--polygon-max-edges", str(ALL_EDGES)]
    generate.main(base + ["--out", os.path.join(root, "exact"), "--polygons", "--polygon-iou"])
    generate.main(base + ["--out", os.path.join(root, "eps"), "--polygon-epsilon", "2", "--polygon-iou"])
    relabel.main(["--ins", os.path.join(root, "exact"), "--out", os.path.join(root, "re_rle")] + poly[:2])
    relabel.main(["--ins", os.path.join(root, "exact"), "--out", os.path.join(root, "re_poly"), "--masks-from", "polygons"] + poly[:2])
    relabel.main(["--ins", os.path.join(root, "eps"), "--out", os.path.join(root, "re_eps"), "--masks-from", "polygons", "--polygons",
                  "--polygon-iou"] + poly)

    # generate: the key and the JSON; without a tolerance every IoU is exactly 1
    ious = []
    for sub, eps in (("exact", 0.0), ("eps", 2.0)):
        per = [e["polygon_iou"] for it in items for e in _load(root, sub, it.key)]
        with open(os.path.join(root, sub, "statistic", "polygon_iou.json")) as f:
            js = json.load(f)
        assert js["n"] == len(per) == 6 and js["polygon_epsilon"] == eps and js["min"] == min(per)
        assert abs(js["average"] - sum(per) / len(per)) < 1e-12 and js["min"] <= js["area"] <= 1.0
        ious.append(per)
    assert ious[0] == [1.0] * 6 and all(0.0 < v < 1.0 for v in ious[1])

    for it in items:
        h, w = it.image.shape[:2]
        # the traced rings are the masks: gray maps, areas and RLE strings byte for byte those of the RLE route
        a, b = _load(root, "re_rle", it.key), _load(root, "re_poly", it.key)
        assert [e["mask"] for e in a] == [e["mask"] for e in b] == [e["mask"] for e in _load(root, "exact", it.key)]
        assert [e["size"] for e in a] == [e["size"] for e in b]
        for kind in ("gray", "color"):
            assert _read(root, "re_rle", kind, it.key) == _read(root, "re_poly", kind, it.key) == _read(root, "exact", kind, it.key)
        # the simplified rings: the masks are their fill, the map is painted from them in order, a later entry wins
        src, got = _load(root, "eps", it.key), _load(root, "re_eps", it.key)
        seg = np.full((h, w), 255, np.uint8)
        for e, g in zip(src, got):
            fill = polygons.rasterize_any([(p, False) for p in e["polygons"]], h, w)
            assert np.array_equal(rle.decode(g["mask"]).astype(np.uint8), fill) and g["size"] == int(fill.sum())
            seg[fill != 0] = int(e["label"])
            assert g["polygon_iou"] == 1.0                           # its own rings, traced again, fill to itself
        assert np.array_equal(np.array(Image.open(os.path.join(root, "re_eps", "gray", f"{it.key}.png"))), seg)

    # an entry without rings (a mask over the edge cap) falls back to its RLE, among entries that are filled
    mixed = _load(root, "exact", items[0].key)
    mixed[1]["polygons"] = mixed[1]["polygon_holes"] = None
    os.makedirs(os.path.join(root, "mixed"))
    with open(os.path.join(root, "mixed", "B0000.pkl"), "wb") as f:
        pickle.dump(mixed, f)
    relabel.main(["--ins", os.path.join(root, "mixed"), "--out", os.path.join(root, "re_mixed"), "--masks-from", "polygons"] + poly[:2])
    assert [e["mask"] for e in _load(root, "re_mixed", "B0000")] == [e["mask"] for e in mixed]
    assert _read(root, "re_mixed", "gray", "B0000") == _read(root, "exact", "gray", "B0000")

    # rings that cannot be filled are an error that names the entry, as an RLE that does not decode is
    wild = _load(root, "exact", items[0].key)
    wild[2]["polygons"] = [np.array([[0, 0], [(1 << 20) + 5, 0], [0, 40]], np.int32)]
    os.makedirs(os.path.join(root, "wild"))
    with open(os.path.join(root, "wild", "B0000.pkl"), "wb") as f:
        pickle.dump(wild, f)
    with pytest.raises(ValueError, match="B0000.pkl.*of entry 2 cannot be filled"):
        relabel.main(["--ins", os.path.join(root, "wild"), "--out", os.path.join(root, "re_wild"), "--masks-from", "polygons"] + poly[:2])

    # an entry with neither rings nor a mask is named
    broken = _load(root, "exact", items[0].key)
    del broken[1]["mask"]
    broken[1]["polygons"] = None
    os.makedirs(os.path.join(root, "broken"))
    with open(os.path.join(root, "broken", "B0000.pkl"), "wb") as f:
        pickle.dump(broken, f)
    with pytest.raises(ValueError, match="entry 1 of B0000 has neither"):
        relabel.main(["--ins", os.path.join(root, "broken"), "--out", os.path.join(root, "re_broken"), "--masks-from", "polygons"] + poly[:2])
