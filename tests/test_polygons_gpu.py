"""GPU: samrs_mask_polygons (polygon_kernels.hip: segment edge masks, scan, link, pointer doubling on the uncut cycles, rank, ring
scan, scatter, corner scan, placement, emit) against the host restatement tests/polygon_ref.py -- the compact edge list with its
successors and corner flags, the leader and rank of every edge (samrs_k_polygon_edges / samrs_k_polygon_ranks) and the call end to
end -- then the option through the tile pipeline, the scene pipeline and the generation CLI.  Integer work on both sides: every
comparison is exact.

Shapes: a lane owns 16 pixels of a row, so 67 x 93 (odd: the byte path, a partial last segment) and 70 x 272 (the 16-byte path),
1 x 1, 1 x 40, 40 x 1; 33 masks for the placement walk; 96 x 96 and 130 x 130 constructed masks (more than one tile of the per-mask
scans: a tile is 4096 entries); a one-pixel-wide spiral, whose single ring needs every doubling round; 1024 x 1024 once."""
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
import region_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N_CLASSES = 18


def _sam(name="vit_tiny", **kw):
    import samrs_amd
    return samrs_amd.sam_model_registry[name](**kw).to("cuda")


@pytest.fixture(scope="module")
def eng():
    sam = _sam(max_images=1, max_prompts=4)
    yield sam.engine


def _buffers(vcap, rcap, cursor=(0, 0)):
    v = torch.full((vcap, 2), -7, dtype=torch.int32, device="cuda")
    r = torch.full((rcap, 4), -7, dtype=torch.int32, device="cuda")
    c = torch.tensor(list(cursor), dtype=torch.int64, device="cuda")
    return v, r, c


def _check_stages(eng, masks, max_edges, what=""):
    d = torch.from_numpy(np.ascontiguousarray(masks)).cuda()
    counts, ids, succ, corner, leader, rank = (t.cpu().numpy() for t in eng.polygon_stages(d, max_edges))
    for j, m in enumerate(masks):
        wi, ws, wc = polygon_ref.edges(m)
        assert int(counts[j]) == wi.size, f"{what} mask {j}: {int(counts[j])} edges, want {wi.size}"
        if wi.size > max_edges:
            continue
        k = wi.size
        assert np.array_equal(ids[j, :k], wi), f"{what} mask {j}: edge ids"
        assert np.array_equal(succ[j, :k], ws), f"{what} mask {j}: successors"
        assert np.array_equal(corner[j, :k], wc), f"{what} mask {j}: corner flags"
        wl, wr = polygon_ref.walk(wi, ws)
        assert np.array_equal(leader[j, :k], wl), f"{what} mask {j}: ring leaders"
        assert np.array_equal(rank[j, :k], wr), f"{what} mask {j}: ranks"


def _check_call(eng, masks, offset=(0, 0), max_edges=65536, vcap=None, rcap=None, cursor=(0, 0), bufs=None, what=""):
    """the call end to end against polygon_ref.mask_polygons; returns (vertices, rings, cursor, table) as numpy and the buffers"""
    d = torch.from_numpy(np.ascontiguousarray(masks)).cuda()
    want_v, want_r, want_c, want_t = polygon_ref.mask_polygons(masks, offset[0], offset[1], max_edges,
                                                               vcap if vcap is not None else 1 << 40,
                                                               rcap if rcap is not None else 1 << 40, cursor)
    if bufs is None:
        bufs = _buffers(vcap if vcap is not None else len(want_v) + 3, rcap if rcap is not None else len(want_r) + 3, cursor)
    v, r, c = bufs
    _, _, _, t = eng.mask_polygons(d, offset, max_edges, v, r, c)
    torch.cuda.synchronize()
    gv, gr, gc, gt = v.cpu().numpy(), r.cpu().numpy(), c.cpu().numpy(), t.cpu().numpy()
    assert gt.tolist() == want_t.tolist(), f"{what}: table {gt.tolist()} want {want_t.tolist()}"
    assert tuple(gc.tolist()) == tuple(want_c), f"{what}: cursor {gc.tolist()} want {want_c}"
    a, b = int(cursor[0]), int(cursor[1])
    assert np.array_equal(gr[b:want_c[1]], want_r[b:]), f"{what}: ring records"
    assert np.array_equal(gv[a:want_c[0]], want_v[a:]), f"{what}: vertices"
    assert (gv[want_c[0]:] == -7).all() and (gr[want_c[1]:] == -7).all(), f"{what}: written behind the cursor"
    return (gv, gr, gc, gt), bufs


def _check(eng, masks, offset=(0, 0), max_edges=65536, what=""):
    _check_stages(eng, masks, max_edges, what)
    (gv, gr, gc, gt), _ = _check_call(eng, masks, offset, max_edges, what=what)
    for j, m in enumerate(masks):
        rl = polygons.rings_of(gt, gr, gv, j)
        if rl is not None:
            assert np.array_equal(polygons.rasterize(rl, m.shape[0], m.shape[1], offset), (m != 0).astype(np.uint8)), f"{what} mask {j}: rasterize"
    return gv, gr, gt


@pytest.mark.parametrize("shape", [(5, 67, 93), (3, 70, 272)])
@pytest.mark.parametrize("density", [0.02, 0.5])
def test_random_masks_byte_path_and_16_byte_path(eng, shape, density):
    rng = np.random.default_rng(int(density * 100) + shape[2])
    masks = (rng.random(shape) < density).astype(np.uint8)
    masks[masks != 0] = rng.integers(1, 256, int(masks.sum()), dtype=np.uint8)        # any non-zero byte is a set pixel
    _check(eng, masks, what=f"{shape} p={density}")


def test_smallest_shapes_and_many_masks_in_one_call(eng):
    gv, gr, gt = _check(eng, np.ones((1, 1, 1), np.uint8), what="1 x 1 set")
    assert gt.tolist() == [[0, 1, 0, 4, 4]] and gr[0].tolist() == [0, 4, 2, 0] and gv[:4].tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]]
    gv, gr, gt = _check(eng, np.zeros((1, 1, 1), np.uint8), what="1 x 1 unset")
    assert gt.tolist() == [[0, 0, 0, 0, 0]]
    rng = np.random.default_rng(7)
    _check(eng, (rng.random((2, 1, 40)) < 0.3).astype(np.uint8), what="1 x 40")
    _check(eng, (rng.random((2, 40, 1)) < 0.3).astype(np.uint8), what="40 x 1")
    many = (rng.random((33, 20, 37)) < 0.1).astype(np.uint8)
    many[5] = 0
    gv, gr, gt = _check(eng, many, what="33 masks")
    assert gt[5, 1] == 0 and gt[5, 3] == 0 and gt[5, 4] == 0 and gt[5, 0] == gt[6, 0] and gt[5, 2] == gt[6, 2]


def _constructed(side: int):
    yy, xx = np.mgrid[0:side, 0:side]
    out = {"empty": np.zeros((side, side), np.uint8), "full": np.ones((side, side), np.uint8)}
    frame = np.ones((side, side), np.uint8)
    frame[3:-3, 3:-3] = 0
    out["frame"] = frame
    out["checkerboard"] = ((yy + xx) % 2 == 0).astype(np.uint8)
    r2 = (yy - side / 2) ** 2 + (xx - side / 2) ** 2
    out["annulus"] = ((r2 <= (0.45 * side) ** 2) & (r2 >= (0.25 * side) ** 2)).astype(np.uint8)
    isl = (r2 <= (0.45 * side) ** 2).astype(np.uint8)
    isl[r2 <= (0.3 * side) ** 2] = 0
    isl[r2 <= (0.12 * side) ** 2] = 1
    out["island in a hole in a blob"] = isl
    out["diagonal"] = np.eye(side, dtype=np.uint8)
    out["anti-diagonal"] = np.ascontiguousarray(np.eye(side, dtype=np.uint8)[:, ::-1])
    return out


@pytest.mark.parametrize("side", [96, 130])
def test_constructed_masks(eng, side):
    shapes = _constructed(side)
    names = list(shapes)
    masks = np.stack(list(shapes.values()))
    gv, gr, gt = _check(eng, masks, what=f"{side} x {side} " + " | ".join(names))
    t = {k: gt[i] for i, k in enumerate(names)}
    assert t["empty"][[1, 3, 4]].tolist() == [0, 0, 0] and t["full"][[1, 3, 4]].tolist() == [1, 4, 4 * side]
    assert t["frame"][1] == 2 and t["annulus"][1] == 2 and t["island in a hole in a blob"][1] == 3
    assert t["diagonal"][[1, 3]].tolist() == [1, 4 * side] and t["anti-diagonal"][[1, 3]].tolist() == [1, 4 * side]
    cb = t["checkerboard"]                                          # one 8-connected component; every interior unset pixel is a hole
    assert cb[1] == 1 + (side - 2) * (side - 2) // 2 and cb[4] == 4 * (side * side // 2)
    rl = polygons.rings_of(gt, gr, gv, names.index("island in a hole in a blob"))
    assert [r[1] for r in rl] == [False, True, False]
    nested = polygons.nest(rl)
    assert len(nested) == 2 and len(nested[0][1]) == 1 and nested[1][1] == []


@pytest.mark.parametrize("side", [96, 130])
def test_spiral_needs_every_doubling_round_and_the_edge_cap(eng, side):
    sp = polygon_ref.spiral(side)
    ne = polygon_ref.count_edges(sp)
    masks = np.stack([sp, np.ascontiguousarray(sp[::-1, ::-1])])
    gv, gr, gt = _check(eng, masks, max_edges=ne + 1, what=f"spiral {side}, cap {ne + 1}")
    assert gt[0, 1] == 1 and gt[0, 4] == ne and gr[0, 1] == gt[0, 3]          # one ring carries every edge
    _check(eng, masks, max_edges=ne, what=f"spiral {side}, cap = its edge count")
    below = 1 << (ne.bit_length() - 1)                              # the next power of two below: over the cap
    assert below < ne
    small = np.zeros((side, side), np.uint8)
    small[5:9, 5:9] = 1
    gv, gr, gt = _check(eng, np.stack([sp, small]), max_edges=below, what=f"spiral {side}, cap {below}")
    assert gt[0].tolist() == [-1, -1, -1, -1, ne] and gt[1].tolist() == [0, 1, 0, 4, 16]


def test_offset_shifts_the_vertices_only(eng):
    rng = np.random.default_rng(11)
    masks = (rng.random((2, 96, 96)) < 0.3).astype(np.uint8)
    v0, r0, t0 = _check(eng, masks)
    v1, r1, t1 = _check(eng, masks, offset=(1000, 31000), what="offset (1000, 31000)")
    k = int(t0[1, 2] + t0[1, 3])
    assert np.array_equal(v1[:k] - v0[:k], np.tile(np.array([1000, 31000], np.int32), (k, 1)))
    assert np.array_equal(r1[:int(t0[1, 0] + t0[1, 1])], r0[:int(t0[1, 0] + t0[1, 1])]) and np.array_equal(t0, t1)
    _check(eng, masks, offset=(32768 - 96, 32768 - 96), what="the largest offset")


def test_two_calls_append_behind_one_cursor(eng):
    rng = np.random.default_rng(13)
    a = (rng.random((3, 40, 52)) < 0.2).astype(np.uint8)
    b = (rng.random((2, 33, 47)) < 0.4).astype(np.uint8)
    (v, r, c, ta), bufs = _check_call(eng, a, vcap=6000, rcap=2000, what="first call")
    before_v, before_r = v[:c[0]].copy(), r[:c[1]].copy()
    (v2, r2, c2, tb), _ = _check_call(eng, b, offset=(5, 9), vcap=6000, rcap=2000, cursor=tuple(c.tolist()), bufs=bufs, what="second call")
    assert np.array_equal(v2[:c[0]], before_v) and np.array_equal(r2[:c[1]], before_r)      # the first call's output is untouched
    assert tb[0, 0] == c[1] and tb[0, 2] == c[0]


def test_capacity_overflow_in_the_middle_of_a_call(eng):
    rng = np.random.default_rng(17)
    masks = (rng.random((5, 30, 44)) < 0.15).astype(np.uint8)
    masks[3] = 0
    masks[3, 4:6, 4:6] = 1                                          # one ring, four vertices: fits where mask 2 did not
    _, _, _, full = polygon_ref.mask_polygons(masks)
    # vertices: room for masks 0, 1 and 4 vertices more
    vcap = int(full[0, 3] + full[1, 3] + 4)
    (v, r, c, t), _ = _check_call(eng, masks, vcap=vcap, rcap=4000, what="vertex capacity")
    assert t[2].tolist() == [-1, -1 - full[2, 1], -1, -1 - full[2, 3], full[2, 4]] and t[3, 1] == 1 and t[3, 3] == 4 and t[4, 1] < 0
    rcap = int(full[0, 1] + full[1, 1] + 1)
    (v, r, c, t), _ = _check_call(eng, masks, vcap=60000, rcap=rcap, what="ring capacity")
    assert t[2].tolist() == [-1, -1 - full[2, 1], -1, -1 - full[2, 3], full[2, 4]] and t[3, 1] == 1 and t[4, 1] < 0
    (v, r, c, t), _ = _check_call(eng, masks, vcap=1, rcap=1, what="no room at all")
    assert (t[:, 0] == -1).all() and (t[:, 1] < -1).all() and c.tolist() == [0, 0]


def test_unaligned_base_takes_the_byte_path_and_agrees(eng):
    rng = np.random.default_rng(5)
    masks = (rng.random((3, 70, 272)) < 0.3).astype(np.uint8)
    buf = torch.zeros(masks.size + 16, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + masks.size].view(3, 70, 272)
    view.copy_(torch.from_numpy(masks).cuda())
    assert view.data_ptr() % 16 == 1 and view.is_contiguous()
    want_v, want_r, want_c, want_t = polygon_ref.mask_polygons(masks)
    v, r, c, t = eng.mask_polygons(view)
    assert t.cpu().tolist() == want_t.tolist() and c.cpu().tolist() == list(want_c)
    assert np.array_equal(v.cpu().numpy()[:want_c[0]], want_v) and np.array_equal(r.cpu().numpy()[:want_c[1]], want_r)


def test_full_size_call(eng):
    masks = np.stack([region_ref.speckled_ellipse(3), polygon_ref.ellipse(1024, 330, 240)])
    gv, gr, gt = _check(eng, masks, what="1024 x 1024")
    assert 20000 < gt[0, 4] < 24000 and gt[1, 1] == 1


def test_bad_arguments_leave_the_outputs_untouched(eng):
    from samrs_amd import engine
    lib, h = eng.lib, eng.handle
    m = torch.ones(2, 8, 8, dtype=torch.uint8, device="cuda")
    v, r, c = _buffers(64, 16)
    t = torch.full((2, 5), -7, dtype=torch.int64, device="cuda")

    def call(masks, n, hh, ww, x0, y0, me, vv=v, rr=r, cc=c, tt=t):
        rc = lib.samrs_mask_polygons(h, masks, n, hh, ww, x0, y0, me, None if vv is None else vv.data_ptr(), 64,
                                     None if rr is None else rr.data_ptr(), 16, None if cc is None else cc.data_ptr(),
                                     None if tt is None else tt.data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    p = m.data_ptr()
    for args in ((p, -1, 8, 8, 0, 0, 64), (None, 2, 8, 8, 0, 0, 64), (p, 2, 0, 8, 0, 0, 64), (p, 2, 8, 0, 0, 0, 64), (p, 2, 8193, 8, 0, 0, 64),
                 (p, 2, 8, 8193, 0, 0, 64), (p, 2, 8, 8, 32761, 0, 64), (p, 2, 8, 8, 0, -1, 64), (p, 2, 8, 8, 0, 0, 3)):
        assert call(*args) == engine.ERR_BAD_ARG, args
    for kw in (dict(vv=None), dict(rr=None), dict(cc=None), dict(tt=None)):
        assert call(p, 2, 8, 8, 0, 0, 64, **kw) == engine.ERR_BAD_ARG, kw
    assert (v == -7).all() and (r == -7).all() and (t == -7).all() and c.cpu().tolist() == [0, 0]
    assert call(p, 0, 8, 8, 0, 0, 64) == engine.OK                  # n == 0 is a no-op
    assert (v == -7).all() and (t == -7).all() and c.cpu().tolist() == [0, 0]
    assert call(p, 2, 8, 8, 0, 0, 64) == engine.OK
    assert t.cpu().tolist() == [[0, 1, 0, 4, 32], [1, 1, 4, 4, 32]] and c.cpu().tolist() == [8, 2]
    assert v[:8].cpu().tolist() == [[0, 0], [8, 0], [8, 8], [0, 8]] * 2 and r[:2].cpu().tolist() == [[0, 4, 128, 0]] * 2
    with pytest.raises(ValueError):
        eng.mask_polygons(m[0])
    with pytest.raises(ValueError):
        eng.mask_polygons(m, max_edges=3)
    with pytest.raises(ValueError):
        eng.mask_polygons(m, vertices=torch.zeros(8, 2, dtype=torch.int64, device="cuda"))


# ------------------------------------------------------------------------------------------------
# the option through the pipelines
# ------------------------------------------------------------------------------------------------
SIZES = [(1024, 1024), (600, 800)]
# the masks of a random-init model are noise with far more edges than the default cap: no 1024^2 mask has more than 2^21
ALL_EDGES = 1 << 21


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
            r.polys = [r.polygons(j) for j in range(len(r.labels))] if r.polygon_table is not None else None
            r.polygon_table = None if r.polygon_table is None else r.polygon_table.copy()
            r.seg_mask = None if r.seg_mask is None else r.seg_mask.copy()
            r.rle_data = r.png_data = r.polygon_rings = r.polygon_vertices = None
            got[r.key] = r
        release()

    pipe.run(batches, sink)
    return got


@pytest.mark.parametrize("batch_decode", [False, True])
def test_tile_pipeline_polygons_rasterize_to_the_masks_that_go_out(batch_decode):
    from samrs_amd import driver, rle
    sam = _sam(max_images=4, max_prompts=20, precision="f16")
    items = _items(driver)
    kw = dict(batch=2, box_batch=3, max_boxes=8, rle=True, rle_buffer_mb=64, min_region_area=16, batch_decode=batch_decode, mask_boxes=True)
    on = _collect(driver.TilePipeline(sam, N_CLASSES, polygons=True, polygon_buffer_mb=64, polygon_max_edges=ALL_EDGES, **kw),
                  driver.batched(items, 2))
    p0 = driver.TilePipeline(sam, N_CLASSES, **kw)
    off = _collect(p0, driver.batched(items, 2))
    assert not hasattr(p0, "poly_vert_dev")                         # off: nothing allocated
    for it in items:
        a, b = on[it.key], off[it.key]
        assert b.polygon_table is None and b.polys is None
        for f in ("seg_mask", "areas", "rle_table", "changed", "mask_hbox", "mask_rbox", "mask_record"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f      # everything else is unchanged
        assert a.rles == b.rles
        h, w = a.size
        for j in range(len(a.labels)):
            mask = rle.decode(a.rles[j]).astype(np.uint8)
            assert a.polys[j] is not None
            assert np.array_equal(polygons.rasterize(a.polys[j], h, w), mask), f"{it.key} instance {j}"
            assert a.polygon_table[j, 4] == polygon_ref.count_edges(mask) and a.polygon_table[j, 3] == sum(len(p[0]) for p in a.polys[j])
            if j == 0:                                               # the host walk of such a mask takes a second: one per tile
                v, r, ne = polygon_ref.trace(mask)
                assert a.polygon_table[j, [1, 3, 4]].tolist() == [len(r), len(v), ne]
                assert np.array_equal(np.concatenate([p[0] for p in a.polys[j]] + [np.zeros((0, 2), np.int32)]), v)


def test_tile_pipeline_edge_cap_gives_none_and_a_small_buffer_raises():
    from samrs_amd import driver
    sam = _sam(max_images=4, max_prompts=20, precision="f16")
    items = _items(driver)[:1]
    kw = dict(batch=2, box_batch=4, max_boxes=8, rle=True, rle_buffer_mb=64)
    r = _collect(driver.TilePipeline(sam, N_CLASSES, polygons=True, polygon_max_edges=4, **kw), driver.batched(items, 2))[items[0].key]
    assert all(p is None or p == [] for p in r.polys) and any(p is None for p in r.polys)
    assert (r.polygon_table[:, 4] >= 0).all()
    with pytest.raises(ValueError):
        driver.InstancePipeline(sam, 1, prompt="box", polygons=True)

    class Tiny(driver.TilePipeline):                                # a buffer of three vertices: the first non-empty mask overflows it
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.poly_vert_dev = [t[:3] for t in self.poly_vert_dev]

    with pytest.raises(RuntimeError, match="polygon_buffer_mb"):
        _collect(Tiny(sam, N_CLASSES, polygons=True, polygon_buffer_mb=1, polygon_max_edges=ALL_EDGES, **kw), driver.batched(items, 2))


def test_scene_pipeline_polygons_are_in_the_scene_frame():
    from samrs_amd import driver, rle
    from samrs_amd.scene import ScenePipeline
    sam = _sam(max_images=8, max_prompts=64, precision="f16")
    H, W = 256, 448
    image = synth.make_image(33, H, W)
    boxes = np.array([[20, 30, 120, 200], [300, 40, 430, 180], [330, 100, 440, 250], [10, 10, 60, 60]], dtype=np.float32)
    labels = np.array([1, 2, 3, 4])
    kw = dict(window=256, overlap=64, batch=2, box_batch=3, rle=True, rle_buffer_mb=16)
    r = _collect(ScenePipeline(sam, N_CLASSES, polygons=True, polygon_buffer_mb=16, polygon_max_edges=ALL_EDGES, **kw),
                 [driver.WorkItem("scene", image, boxes, labels)])["scene"]
    off = _collect(ScenePipeline(sam, N_CLASSES, **kw), [driver.WorkItem("scene", image, boxes, labels)])["scene"]
    assert off.polygon_table is None and off.rles == r.rles and np.array_equal(off.seg_mask, r.seg_mask)
    assert len(r.windows) == 2 and r.windows[1][0] > 0 and sorted(set(r.window_of)) == [0, 1]
    for j in range(4):
        pasted = rle.decode(r.rles[j]).astype(np.uint8)             # the mask pasted at its window's offset: the scene frame
        assert pasted.shape == (H, W)
        assert np.array_equal(polygons.rasterize(r.polys[j], H, W), pasted), f"scene instance {j}"
        if j == 0:
            v, rr, ne = polygon_ref.trace(pasted)
            assert np.array_equal(np.concatenate([p[0] for p in r.polys[j]] + [np.zeros((0, 2), np.int32)]), v)


def test_generate_cli_writes_the_pickle_keys(tmp_path):
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
    generate.main(base + ["--out", str(tmp_path / "on"), "--polygons", "--polygon-buffer-mb", "64", "--polygon-max-edges", str(ALL_EDGES),
                         "--log", str(tmp_path / "log.jsonl")])
    generate.main(base + ["--out", str(tmp_path / "off")])
    for it in items:
        with open(tmp_path / "on" / "ins" / f"{it.key}.pkl", "rb") as f:
            info = pickle.load(f)
        with open(tmp_path / "off" / "ins" / f"{it.key}.pkl", "rb") as f:
            plain = pickle.load(f)
        for e, q in zip(info, plain):
            mask = rle.decode(e["mask"]).astype(np.uint8)
            assert len(e["polygons"]) == len(e["polygon_holes"]) and all(p.dtype == np.int32 and p.shape[1] == 2 for p in e["polygons"])
            assert np.array_equal(polygons.rasterize(list(zip(e["polygons"], e["polygon_holes"])), *mask.shape), mask)
            stripped = {k: v for k, v in e.items() if k not in ("polygons", "polygon_holes")}
            assert sorted(stripped) == sorted(q) and stripped["mask"] == q["mask"] and stripped["size"] == q["size"]
        for sub in ("gray", "color"):
            assert open(tmp_path / "on" / sub / f"{it.key}.png", "rb").read() == open(tmp_path / "off" / sub / f"{it.key}.png", "rb").read()
    lines = [json.loads(l) for l in open(tmp_path / "log.jsonl").read().splitlines()]
    assert any(l.get("polygons_over_cap") == [0, 0] for l in lines)
