"""GPU: samrs_simplify_polygons (polygon_simplify_kernels.hip: the rows' rings listed, the Douglas-Peucker rounds per ring in three
grades -- one wave, one workgroup in LDS, one workgroup over global scratch --, the scan of the kept counts and the compaction through
the staging copy) against the host statement tests/polygon_simplify_ref.py applied to the un-simplified output of the same call:
vertices, ring records, table and cursor bit for bit, and the checker's three properties on every ring, independently of that.  Then
the option through the tile pipeline, the scene pipeline, generate and relabel.

Shapes: the random masks of the tracing tests (5, 67, 93); 64 x 64 constructed masks; combs whose single ring has exactly 64 / 68 and
2048 / 2052 vertices (the two switches between the grades: PS_WAVE_MAX = 64, PS_LDS_MAX = 2048); a disc whose staircase needs more
than 8 nested splits (the in-kernel loop over rounds)."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from samrs_amd import polygons, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polygon_ref  # noqa: E402
import polygon_simplify_ref as ps_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N_CLASSES = 18
FILL = -7


def _sam(name="vit_tiny", **kw):
    import samrs_amd
    return samrs_amd.sam_model_registry[name](**kw).to("cuda")


@pytest.fixture(scope="module")
def eng():
    sam = _sam(max_images=1, max_prompts=4)
    yield sam.engine


def _buffers(vcap, rcap, cursor=(0, 0)):
    v = torch.full((vcap, 2), FILL, dtype=torch.int32, device="cuda")
    r = torch.full((rcap, 4), FILL, dtype=torch.int32, device="cuda")
    c = torch.tensor(list(cursor), dtype=torch.int64, device="cuda")
    return v, r, c


def _np(*ts):
    return [t.cpu().numpy().copy() for t in ts]


def _properties(t0, r0, v0, t1, r1, v1, eps_q, what):
    """test 8: the checker on every ring of every placed row, before against after"""
    for j in range(len(t0)):
        before, after = polygons.rings_of(t0, r0, v0, j), polygons.rings_of(t1, r1, v1, j)
        assert (before is None) == (after is None), f"{what} row {j}"
        if before is None:
            continue
        assert len(before) == len(after)
        for q, (b, a) in enumerate(zip(before, after)):
            assert b[1] == a[1], f"{what} row {j} ring {q}: hole flag"
            assert ps_ref.check_ring(b[0], a[0], eps_q), f"{what} row {j} ring {q}"


def _simplify_and_check(eng, table, v, r, c, eps_q, what="", stages=True):
    """one simplify over the rows of `table` (device tensors; v, r, c the shared buffers): everything against the host statement of
    the buffers as they are now.  Returns (table, rings, vertices, cursor) as numpy after the call and the statement's depth."""
    t0, r0, v0, c0 = _np(table, r, v, c)
    wt, wr, wv, wc, depth = ps_ref.simplify_buffers(t0, r0, v0, c0, eps_q)
    if stages and len(t0):
        keep, kept = (x.cpu().numpy() for x in eng.polygon_simplify_stages(table, r, v, eps_q))
        assert np.array_equal(_np(table, r, v, c)[1], r0) and np.array_equal(v.cpu().numpy(), v0), f"{what}: the stage hook wrote"
        want_keep, want_kept = np.zeros(len(v0), np.uint8), np.full(len(r0), -1, np.int32)
        for j in range(len(t0)):
            if not ps_ref.row_placed(t0[j]):
                continue
            for q in range(int(t0[j, 0]), int(t0[j, 0] + t0[j, 1])):
                a, k = int(t0[j, 2]) + int(r0[q, 0]), int(r0[q, 1])
                idx, _ = ps_ref.simplify_ring(v0[a:a + k], eps_q)
                want_keep[[a + i for i in idx]] = 1
                want_kept[q] = len(idx)
        assert np.array_equal(kept, want_kept), f"{what}: kept counts per ring"
        assert np.array_equal(keep, want_keep), f"{what}: keep flags"
    eng.simplify_polygons(table, r, v, c, eps_q / 16.0)
    torch.cuda.synchronize()
    t1, r1, v1, c1 = _np(table, r, v, c)
    assert c1.tolist() == wc.tolist(), f"{what}: cursor {c1.tolist()} want {wc.tolist()}"
    assert t1.tolist() == wt.tolist(), f"{what}: table"
    assert np.array_equal(r1, wr), f"{what}: ring records"
    assert np.array_equal(v1, wv), f"{what}: vertices"
    _properties(t0, r0, v0, t1, r1, v1, eps_q, what)
    return (t1, r1, v1, c1), depth


def _trace(eng, masks, offset=(0, 0), bufs=None, max_edges=65536, slack=5):
    d = torch.from_numpy(np.ascontiguousarray(masks)).cuda()
    if bufs is None:
        want_v, want_r, _, _ = polygon_ref.mask_polygons(masks, offset[0], offset[1], max_edges)
        bufs = _buffers(len(want_v) + slack, len(want_r) + slack)
    v, r, c = bufs
    _, _, _, t = eng.mask_polygons(d, offset, max_edges, v, r, c)
    return t, bufs


def _run(eng, masks, eps_q, offset=(0, 0), what=""):
    t, (v, r, c) = _trace(eng, masks, offset)
    return _simplify_and_check(eng, t, v, r, c, eps_q, what)


# ------------------------------------------------------------------------------------------------
# constructed masks
# ------------------------------------------------------------------------------------------------
def _disc(side, radius, hole=0.0):
    yy, xx = np.mgrid[0:side, 0:side]
    r2 = (yy - side / 2 + 0.5) ** 2 + (xx - side / 2 + 0.5) ** 2
    return ((r2 <= radius * radius) & (r2 >= hole * hole)).astype(np.uint8)


def _staircase_triangle(side=64):
    yy, xx = np.mgrid[0:side, 0:side]
    return ((xx <= yy) & (yy < side - 4) & (xx >= 3)).astype(np.uint8)


def _comb(teeth, seed=0):
    """a one-pixel bar with `teeth` one-pixel teeth of 1 .. 6 pixels on it: one ring of 4 + 4 teeth vertices"""
    rng = np.random.default_rng(seed)
    m = np.zeros((8, 2 * teeth + 2), np.uint8)
    m[7, :] = 1
    for i, hgt in enumerate(rng.integers(1, 7, teeth)):
        m[7 - hgt:7, 2 * i + 1] = 1
    return m


def _constructed():
    side = 64
    out = {}
    one = np.zeros((side, side), np.uint8)
    one[30, 41] = 1
    out["single pixel"] = one
    blk = np.zeros((side, side), np.uint8)
    blk[10:12, 20:22] = 1
    out["2 x 2 block"] = blk
    line = np.zeros((side, side), np.uint8)
    line[17, 5:60] = 1
    out["one-pixel line"] = line
    out["disc with a hole"] = _disc(side, 20, 8)
    out["staircase triangle"] = _staircase_triangle(side)
    sad = np.zeros((side, side), np.uint8)
    sad[8:30, 6:31] = 1
    for i in range(6):
        sad[8 + i, 6:11 - i] = 0                                    # a staircase corner cut from the first blob
    sad[30:50, 31:52] = 1                                           # pixels (29, 30) and (30, 31): the blobs meet at lattice point (31, 30) only
    out["two blobs at a saddle"] = sad
    rng = np.random.default_rng(3)
    sp = np.zeros((side, side), np.uint8)
    ys, xs = np.meshgrid(np.arange(1, side, 2), np.arange(1, side, 2), indexing="ij")
    pick = rng.permutation(ys.size)[:200]
    sp[ys.reshape(-1)[pick], xs.reshape(-1)[pick]] = 1
    out["speckle"] = sp
    return out


def test_constructed_rings_are_what_their_names_say():
    """no GPU work: the masks above have the rings the cases are about"""
    c = _constructed()
    v, r, _ = polygon_ref.trace(c["speckle"])
    assert len(r) == 200 and all(int(x[1]) == 4 for x in r)
    v, r, _ = polygon_ref.trace(c["two blobs at a saddle"])
    assert len(r) == 1 and len({tuple(p) for p in v.tolist()}) == len(v) - 1          # one ring, one lattice point visited twice
    for teeth, k in ((15, 64), (16, 68), (511, 2048), (512, 2052)):
        v, r, _ = polygon_ref.trace(_comb(teeth))
        assert len(r) == 1 and int(r[0][1]) == k == len(v)


@pytest.mark.parametrize("eps_q", [8, 16, 40])
@pytest.mark.parametrize("density", [0.02, 0.5])
def test_random_masks(eng, density, eps_q):
    rng = np.random.default_rng(int(density * 100) + 93)
    masks = (rng.random((5, 67, 93)) < density).astype(np.uint8)
    _run(eng, masks, eps_q, what=f"p={density} eps_q={eps_q}")


@pytest.mark.parametrize("eps_q", [8, 16, 40])
def test_constructed_masks(eng, eps_q):
    shapes = _constructed()
    masks = np.stack([shapes[k] for k in shapes])
    (t1, r1, v1, c1), _ = _run(eng, masks, eps_q, what=f"constructed eps_q={eps_q}")
    names = list(shapes)
    j = names.index("single pixel")
    assert t1[j, 3] == 4 - (eps_q >= 12) and t1[j, 1] == 1           # a unit square: its fourth corner is sqrt(1/2) = 11.3 / 16 away
    j = names.index("speckle")
    assert t1[j, 1] == 200 and t1[j, 3] == 200 * (4 - (eps_q >= 12))
    j = names.index("one-pixel line")
    assert t1[j, 3] == (4 if eps_q < 16 else 3)                      # a 55 x 1 bar: the fourth corner is sqrt(3025 / 3026) of a pixel from the diagonal
    # the third field is the ORIGINAL ring's area: every mask's rings still sum to twice its pixels
    for j, name in enumerate(names):
        a2 = sum(int(r1[q, 2]) for q in range(int(t1[j, 0]), int(t1[j, 0] + t1[j, 1])))
        assert a2 == 2 * int(shapes[name].sum()), name


def test_deep_ring_pins_the_round_loop(eng):
    disc = _disc(128, 60)[None]
    (t1, r1, v1, c1), depth = _run(eng, disc, 8, what="disc of radius 60")
    assert depth >= 8, depth
    assert t1[0, 1] == 1 and 3 < t1[0, 3] < 284


@pytest.mark.parametrize("teeth", [15, 16, 511, 512])
def test_rings_on_both_sides_of_each_grade_switch(eng, teeth):
    for eps_q in (8, 40):
        (t1, r1, v1, c1), _ = _run(eng, _comb(teeth, seed=teeth)[None], eps_q, what=f"comb of {teeth} teeth eps_q={eps_q}")
        assert t1[0, 1] == 1 and 3 <= t1[0, 3] <= 4 + 4 * teeth
    # all three grades in one call, the longest ring in the middle
    masks = np.zeros((3, 8, 2 * 512 + 2), np.uint8)
    masks[0, :, :32] = _comb(15, 1)
    masks[1] = _comb(512, 2)
    masks[2, :, :402] = _comb(200, 3)
    _run(eng, masks, 16, what="three grades")


def test_two_appends_then_one_simplify_then_again_behind_the_rewound_cursor(eng):
    rng = np.random.default_rng(13)
    a = (rng.random((3, 40, 52)) < 0.2).astype(np.uint8)
    b = (rng.random((2, 33, 47)) < 0.4).astype(np.uint8)
    bufs = _buffers(6000, 2000)
    ta, _ = _trace(eng, a, bufs=bufs)
    tb, _ = _trace(eng, b, offset=(5, 9), bufs=bufs)
    v, r, c = bufs
    both = torch.cat([ta, tb])
    (t1, r1, v1, c1), _ = _simplify_and_check(eng, both, v, r, c, 16, what="two tables")
    assert 0 < c1[0] < int(ta[:, 3].sum() + tb[:, 3].sum()) and c1[1] == int(ta[:, 1].sum() + tb[:, 1].sum())
    # a third call appends behind the rewound cursor; the second simplify sees its rows only
    d = (rng.random((2, 30, 30)) < 0.5).astype(np.uint8)
    td, _ = _trace(eng, d, offset=(100, 200), bufs=bufs)
    assert int(td[0, 2]) == int(c1[0]) and int(td[0, 0]) == int(c1[1])
    (t2, r2, v2, c2), _ = _simplify_and_check(eng, td, v, r, c, 24, what="the new rows only")
    assert np.array_equal(v2[:c1[0]], v1[:c1[0]]) and np.array_equal(r2[:c1[1]], r1[:c1[1]])       # the first result is untouched


def test_rows_not_traced_or_not_placed_pass_through(eng):
    rng = np.random.default_rng(17)
    masks = (rng.random((6, 30, 44)) < 0.15).astype(np.uint8)
    masks[2] = (rng.random((30, 44)) < 0.5)                         # over the edge cap below
    masks[4] = 0                                                    # an empty mask in the middle
    masks[5] = 0
    masks[5, 4:6, 4:8] = 1                                          # one ring, four vertices: fits where mask 3 did not
    ne = [polygon_ref.count_edges(m) for m in masks]
    cap = max(ne[j] for j in (0, 1, 3, 5))
    assert ne[2] > cap
    _, _, _, full = polygon_ref.mask_polygons(masks, max_edges=cap)
    # vertices: room for masks 0, 1 and 5, not for 3
    vcap = int(full[0, 3] + full[1, 3] + full[5, 3] + 1)
    assert full[3, 3] > full[5, 3] + 1
    bufs = _buffers(vcap, 4000)
    t, _ = _trace(eng, masks, bufs=bufs, max_edges=cap)
    got = t.cpu().numpy()
    assert got[2, :4].tolist() == [-1, -1, -1, -1] and got[3, 0] == -1 and got[3, 1] < -1 and got[4, 1] == 0 and got[5, 1] > 0
    v, r, c = bufs
    (t1, r1, v1, c1), _ = _simplify_and_check(eng, t, v, r, c, 16, what="rows passed through")
    assert np.array_equal(t1[2], got[2]) and np.array_equal(t1[3], got[3]) and t1[4, 1] == 0 and t1[4, 3] == 0
    assert t1[4, 2] == t1[5, 2] == t1[1, 2] + t1[1, 3]
    # no row placed at all: nothing moves, the cursor included
    bufs = _buffers(1, 1)
    t, _ = _trace(eng, masks[:2], bufs=bufs)
    v, r, c = bufs
    before = _np(t, r, v, c)
    eng.simplify_polygons(t, r, v, c, 1.0)
    torch.cuda.synchronize()
    for x, y in zip(before, _np(t, r, v, c)):
        assert np.array_equal(x, y)


def test_no_rows_and_bad_arguments_leave_every_byte_untouched(eng):
    from samrs_amd import engine
    lib, h = eng.lib, eng.handle
    m = torch.zeros(2, 8, 8, dtype=torch.uint8, device="cuda")
    m[:, 2:5, 1:7] = 1
    m[0, 5, 3] = 1
    t, (v, r, c) = _trace(eng, m.cpu().numpy())
    before = _np(t, r, v, c)

    def call(vv, rr, tt, n, q, cc):
        rc = lib.samrs_simplify_polygons(h, None if vv is None else vv.data_ptr(), None if rr is None else rr.data_ptr(),
                                         None if tt is None else tt.data_ptr(), n, q, None if cc is None else cc.data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    assert call(v, r, t, 0, 16, c) == engine.OK                    # n == 0 is a no-op
    for args in ((None, r, t, 2, 16, c), (v, None, t, 2, 16, c), (v, r, None, 2, 16, c), (v, r, t, 2, 16, None), (v, r, t, -1, 16, c),
                 (v, r, t, 2, 0, c), (v, r, t, 2, -16, c), (v, r, t, 2, 16385, c)):
        assert call(*args) == engine.ERR_BAD_ARG, args
    assert lib.samrs_simplify_polygons(None, v.data_ptr(), r.data_ptr(), t.data_ptr(), 2, 16, c.data_ptr(), None) == engine.ERR_BAD_ARG
    # buffers the handle never traced into: their capacities are unknown (a view at an odd offset: no allocation ever started there)
    other = torch.zeros(v.shape[0] + 1, 2, dtype=torch.int32, device="cuda")[1:]
    assert call(other, r, t, 2, 16, c) == engine.ERR_BAD_ARG
    for x, y in zip(before, _np(t, r, v, c)):
        assert np.array_equal(x, y)
    assert (other == 0).all()
    for eps in (0.0, -1.0, 0.03, 1024.04, float("nan")):
        with pytest.raises(ValueError):
            eng.simplify_polygons(t, r, v, c, eps)
    with pytest.raises(ValueError):
        eng.simplify_polygons(t.to(torch.int32), r, v, c, 1.0)
    for x, y in zip(before, _np(t, r, v, c)):
        assert np.array_equal(x, y)
    assert call(v, r, t, 2, 16384, c) == engine.OK                  # the largest tolerance: every ring down to its anchors
    t1 = t.cpu().numpy()
    assert t1[:, 3].tolist() == [3, 3] and c.cpu().tolist() == [6, 2]


def test_offset_shifts_the_simplified_vertices_only(eng):
    rng = np.random.default_rng(11)
    masks = (rng.random((2, 96, 96)) < 0.3).astype(np.uint8)
    (t0, r0, v0, c0), _ = _run(eng, masks, 16)
    (t1, r1, v1, c1), _ = _run(eng, masks, 16, offset=(1000, 31000), what="offset (1000, 31000)")
    k = int(c0[0])
    assert np.array_equal(t0, t1) and np.array_equal(c0, c1) and np.array_equal(r0[:c0[1]], r1[:c0[1]])
    assert np.array_equal(v1[:k] - v0[:k], np.tile(np.array([1000, 31000], np.int32), (k, 1)))


# ------------------------------------------------------------------------------------------------
# the option through the pipelines and the CLIs
# ------------------------------------------------------------------------------------------------
SIZES = [(256, 320), (192, 256)]    # small tiles: the host statement walks every ring of their (random-init: noise) masks
ALL_EDGES = 1 << 21                 # no mask of these sizes has more edges
EPS = 1.0
OTHER_FIELDS = ("seg_mask", "areas", "rle_table", "changed", "mask_hbox", "mask_rbox", "mask_record")


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
            r.rles = [r.rle(j) for j in range(len(r.labels))] if r.rle_table is not None else None
            r.polys = [r.polygons(j) for j in range(len(r.labels))]
            first_ring = r.polygon_table[:, 0]
            r.ring_tails = [r.polygon_rings[int(f):int(f + n), 2:].copy() for f, n in zip(first_ring, r.polygon_table[:, 1])]
            r.polygon_table = r.polygon_table.copy()
            r.seg_mask = r.seg_mask.copy()
            r.rle_data = r.png_data = r.polygon_rings = r.polygon_vertices = None
            got[r.key] = r
        release()

    pipe.run(batches, sink)
    return got


def _want_rings(rings_list, eps_q):
    return [(np.asarray(p)[ps_ref.simplify_ring_fast(p, eps_q)], hole) for p, hole in rings_list]


def _same_rings(got, want):
    return len(got) == len(want) and all(g[1] == w[1] and np.array_equal(g[0], w[0]) for g, w in zip(got, want))


def _check_results(on, off, eps_q, what):
    """every other output byte-identical; the polygons the host statement of the un-simplified run's polygons"""
    for f in OTHER_FIELDS:
        assert np.array_equal(getattr(on, f), getattr(off, f)), f"{what}: {f}"
    assert on.rles == off.rles
    assert np.array_equal(on.polygon_table[:, [1, 4]], off.polygon_table[:, [1, 4]]), f"{what}: ring and edge counts"
    dropped = 0
    for j in range(len(on.labels)):
        want = _want_rings(off.polys[j], eps_q)
        assert _same_rings(on.polys[j], want), f"{what} instance {j}"
        assert on.polygon_table[j, 3] == sum(len(p[0]) for p in want)
        assert np.array_equal(on.ring_tails[j], off.ring_tails[j]), f"{what} instance {j}: area and pixel of the ring records"
        dropped += int(off.polygon_table[j, 3] - on.polygon_table[j, 3])
        for (b, _), (a, _) in list(zip(off.polys[j], on.polys[j]))[:50]:
            assert ps_ref.check_ring(b, a, eps_q)
    assert dropped > 0, f"{what}: nothing was simplified"


@pytest.mark.parametrize("batch_decode", [False, True])
def test_tile_pipeline_simplifies_the_polygon_stream_and_nothing_else(batch_decode):
    from samrs_amd import driver
    sam = _sam(max_images=4, max_prompts=20, precision="f16")
    items = _items(driver)
    kw = dict(batch=2, box_batch=2, max_boxes=8, rle=True, rle_buffer_mb=16, min_region_area=16, batch_decode=batch_decode, mask_boxes=True,
              polygons=True, polygon_buffer_mb=16, polygon_max_edges=ALL_EDGES)
    pipe = driver.TilePipeline(sam, N_CLASSES, polygon_epsilon=EPS, **kw)
    assert pipe.polygon_eps_q == 16
    on = _collect(pipe, driver.batched(items, 2))
    p0 = driver.TilePipeline(sam, N_CLASSES, polygon_epsilon=0.0, **kw)
    assert p0.polygon_eps_q == 0
    off = _collect(p0, driver.batched(items, 2))
    for it in items:
        _check_results(on[it.key], off[it.key], 16, f"{it.key} batch_decode={batch_decode}")


def test_scene_pipeline_simplifies_in_the_scene_frame():
    from samrs_amd import driver
    from samrs_amd.scene import ScenePipeline
    sam = _sam(max_images=8, max_prompts=64, precision="f16")
    H, W = 256, 448
    image = synth.make_image(33, H, W)
    boxes = np.array([[20, 30, 120, 200], [300, 40, 430, 180], [330, 100, 440, 250], [10, 10, 60, 60]], dtype=np.float32)
    labels = np.array([1, 2, 3, 4])
    kw = dict(window=256, overlap=64, batch=2, box_batch=3, rle=True, rle_buffer_mb=16, min_region_area=16, mask_boxes=True, polygons=True,
              polygon_buffer_mb=16, polygon_max_edges=ALL_EDGES)
    on = _collect(ScenePipeline(sam, N_CLASSES, polygon_epsilon=2.5, **kw), [driver.WorkItem("scene", image, boxes, labels)])["scene"]
    off = _collect(ScenePipeline(sam, N_CLASSES, **kw), [driver.WorkItem("scene", image, boxes, labels)])["scene"]
    assert len(on.windows) == 2 and on.windows[1][0] > 0 and sorted(set(on.window_of)) == [0, 1]
    _check_results(on, off, 40, "scene")
    xs = np.concatenate([p[0][:, 0] for j in range(4) for p in on.polys[j]])
    assert xs.max() > 256                                           # vertices of the second window: the scene's frame
    with pytest.raises(ValueError, match="needs polygons=True"):
        ScenePipeline(sam, N_CLASSES, polygon_epsilon=1.0)
    with pytest.raises(ValueError, match="polygon_epsilon"):
        driver.InstancePipeline(sam, 1, prompt="box", polygon_epsilon=1.0)


def test_generate_writes_the_three_keys_and_relabel_reproduces_them(tmp_path):
    from samrs_amd import driver, generate, relabel, tile_io
    items = _items(driver)
    img_dir = tmp_path / "img"
    img_dir.mkdir()
    ann = {}
    for it in items:
        tile_io.write_rgb(str(img_dir / f"{it.key}.png"), it.image, 1)
        ann[it.key] = {"boxes": it.boxes.tolist(), "labels": it.labels.tolist()}
    (tmp_path / "boxes.json").write_text(json.dumps(ann))
    base = ["--images", str(img_dir), "--boxes", str(tmp_path / "boxes.json"), "--model", "vit_tiny", "--box-batch", "20", "--batch", "2",
            "--polygon-buffer-mb", "16", "--polygon-max-edges", str(ALL_EDGES)]
    generate.main(base + ["--out", str(tmp_path / "on"), "--polygon-epsilon", "1.53"])           # implies --polygons; 1.53 -> 24 / 16
    generate.main(base + ["--out", str(tmp_path / "off"), "--polygons"])
    relabel.main(["--ins", str(tmp_path / "off"), "--out", str(tmp_path / "re"), "--n-classes", str(N_CLASSES), "--polygon-epsilon", "1.53",
                  "--polygon-buffer-mb", "16", "--polygon-max-edges", str(ALL_EDGES)])

    def load(sub, key):
        with open(tmp_path / sub / "ins" / f"{key}.pkl", "rb") as f:
            return pickle.load(f)

    for it in items:
        on, off, re_ = load("on", it.key), load("off", it.key), load("re", it.key)
        assert len(on) == len(off) == len(re_) == len(it.labels)
        for e, q, z in zip(on, off, re_):
            assert e["polygon_epsilon"] == 1.5 and z["polygon_epsilon"] == 1.5 and "polygon_epsilon" not in q
            assert sorted(set(e) - set(q)) == ["polygon_epsilon"] and e["mask"] == q["mask"] == z["mask"] and e["size"] == q["size"]
            want = _want_rings(list(zip(q["polygons"], q["polygon_holes"])), 24)
            for got in (e, z):
                assert got["polygon_holes"] == q["polygon_holes"] and all(p.dtype == np.int32 and p.shape[1] == 2 for p in got["polygons"])
                assert _same_rings(list(zip(got["polygons"], got["polygon_holes"])), want)
        for sub in ("gray", "color"):
            assert open(tmp_path / "on" / sub / f"{it.key}.png", "rb").read() == open(tmp_path / "off" / sub / f"{it.key}.png", "rb").read()
