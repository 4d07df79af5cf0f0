"""CPU: the fill rule of samrs_fill_polygons as two independent host statements (tests/polygon_fill_ref.py: a per-pixel crossing count
over Python ints; samrs_amd.polygons.rasterize_any: a ceiling per edge and row), the host helpers around it (pack_rings,
iou_from_counts), the validation of the `polygon_iou` / `--masks-from` options, and the reduction behind statistic/polygon_iou.json
under gloo with two ranks."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from samrs_amd import driver, polygons

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polygon_fill_ref as pf_ref  # noqa: E402

TIE_TRIANGLE = [(np.array([[0, 0], [8, 8], [0, 8]]), False)]        # its diagonal passes through the centres of pixels (r, r)


def _random_rings(rng, origin, lo=-20, hi=70):
    return [(rng.integers(lo, hi, (int(rng.integers(3, 9)), 2)) + np.asarray(origin), bool(rng.integers(0, 2)))
            for _ in range(int(rng.integers(1, 4)))]


def test_the_two_statements_agree_on_random_rings():
    """vertices outside the window, shifted origins; random rings of up to 8 vertices cross themselves and each other"""
    rng = np.random.default_rng(0)
    crossing = 0
    for _ in range(120):
        h, w = int(rng.integers(1, 30)), int(rng.integers(1, 40))
        origin = (int(rng.integers(0, 50)), int(rng.integers(0, 50)))
        rl = _random_rings(rng, origin)
        want = pf_ref.fill(rl, h, w, origin)
        assert np.array_equal(polygons.rasterize_any(rl, h, w, origin), want), (h, w, origin, rl)
        crossing += int(want.any() and not want.all())
    assert crossing > 60                                             # the cases are not all empty or all full


def test_bow_tie_and_the_tie_rule():
    bow = [(np.array([[1, 1], [9, 9], [9, 1], [1, 9]]), False)]     # self-crossing at (5, 5)
    want = pf_ref.fill(bow, 10, 10)
    assert np.array_equal(polygons.rasterize_any(bow, 10, 10), want)
    assert want[2, 1] == 1 and want[5, 2] == 1 and want[5, 7] == 1 and want[2, 5] == 0 and want[7, 5] == 0   # left and right lobes
    got = pf_ref.fill(TIE_TRIANGLE, 8, 8)
    assert np.array_equal(polygons.rasterize_any(TIE_TRIANGLE, 8, 8), got)
    # the centre (r + 1/2, r + 1/2) lies ON the diagonal: it counts as right of it, so the diagonal edge toggles pixel (r, r) and the
    # left edge x = 0 toggles it too -- the diagonal pixels are out, the ones left of them in
    assert np.array_equal(got, np.tril(np.ones((8, 8), np.uint8), -1))


def test_the_reference_equals_rasterize_on_lattice_rings():
    m = np.zeros((9, 11), np.uint8)
    m[1:8, 2:10] = 1
    m[3:6, 4:8] = 0
    m[4, 5] = 1                                                      # an island inside the hole
    rl = [(np.array([[2, 1], [10, 1], [10, 8], [2, 8]]), False), (np.array([[4, 3], [4, 6], [8, 6], [8, 3]]), True),
          (np.array([[5, 4], [6, 4], [6, 5], [5, 5]]), False)]
    assert np.array_equal(pf_ref.fill(rl, 9, 11), m) and np.array_equal(polygons.rasterize(rl, 9, 11), m)
    assert np.array_equal(pf_ref.fill(rl, 9, 11, origin=(0, 0)), polygons.rasterize_any(rl, 9, 11))
    shifted = [(p + np.array([100, 200]), hole) for p, hole in rl]
    assert np.array_equal(pf_ref.fill(shifted, 9, 11, origin=(100, 200)), m)


def test_rows_that_are_not_rings_in_the_reference():
    far = [(np.array([[0, 0], [(1 << 20) + 1, 0], [0, 5]]), False)]
    assert not pf_ref.placed(far) and not pf_ref.fill(far, 4, 4).any()
    edge = [(np.array([[0, 0], [1 << 20, 0], [0, 5]]), False)]      # exactly 2^20 away: still filled
    assert pf_ref.placed(edge) and pf_ref.fill(edge, 4, 4).any()
    assert not pf_ref.placed(None) and not pf_ref.fill(None, 3, 3).any()
    assert pf_ref.counts(np.zeros((3, 3), np.uint8), np.ones((3, 3), np.uint8), is_rings=False) == [-1, 9, 0]
    assert pf_ref.counts(np.ones((3, 3), np.uint8), None) == [9, 0, 0]


def test_pack_rings_inverts_rings_of():
    # hand-written, in pack_rings's canonical form: row 0 = a square with a hole, row 1 not traced, row 2 empty, row 3 a triangle
    table = np.array([[0, 2, 0, 8, 8], [-1, -1, -1, -1, 0], [2, 0, 8, 0, 0], [2, 1, 8, 3, 3]], np.int64)
    rings = np.array([[0, 4, 32, 0], [4, 4, -8, 0], [0, 3, 16, 0]], np.int32)
    vertices = np.array([[0, 0], [4, 0], [4, 4], [0, 4], [1, 1], [1, 3], [3, 3], [3, 1], [5, 5], [9, 5], [9, 9]], np.int32)
    lists = [polygons.rings_of(table, rings, vertices, j) for j in range(4)]
    assert lists[1] is None and lists[2] == [] and [r[1] for r in lists[0]] == [False, True]
    t, r, v = polygons.pack_rings(lists)
    assert t.dtype == np.int64 and r.dtype == np.int32 and v.dtype == np.int32
    assert np.array_equal(t, table) and np.array_equal(r, rings) and np.array_equal(v, vertices)
    for j in range(4):                                               # and the other way round
        back = polygons.rings_of(t, r, v, j)
        assert (back is None) == (lists[j] is None)
        if back is not None:
            assert len(back) == len(lists[j]) and all(a[1] == b[1] and np.array_equal(a[0], b[0]) for a, b in zip(back, lists[j]))
    # bare vertex arrays are rings too; nothing at all still uploads
    t, r, v = polygons.pack_rings([[np.array([[0, 0], [2, 0], [2, 2]])]])
    assert t.tolist() == [[0, 1, 0, 3, 3]] and r[0, :2].tolist() == [0, 3]
    t, r, v = polygons.pack_rings([None, []])
    assert t[:, 1].tolist() == [-1, 0] and r.shape == (1, 4) and v.shape == (1, 2)
    with pytest.raises(ValueError):
        polygons.pack_rings([[np.zeros((0, 2), np.int32)]])


def test_iou_from_counts():
    got = polygons.iou_from_counts(np.array([[0, 0, 0], [-1, 5, 0], [4, 4, 2], [6, 6, 6], [0, 7, 0]], np.int64))
    assert got.dtype == np.float64 and got[0] == 1.0 and np.isnan(got[1]) and got[2] == 2 / 6 and got[3] == 1.0 and got[4] == 0.0
    assert float(polygons.iou_from_counts(np.array([3, 5, 3]))) == 3 / 5
    assert polygons.iou_from_counts(torch.tensor([[2, 2, 1]])).tolist() == [1 / 3]


def test_option_validation():
    from samrs_amd import relabel
    from samrs_amd.scene import ScenePipeline
    with pytest.raises(ValueError, match="polygon_iou.*needs polygons=True"):
        driver.validate_output_options(polygon_iou=True)
    assert driver.validate_output_options(polygons=True, polygon_iou=True)[1] is not None
    assert driver.validate_output_options(polygon_iou=False) == (None, None)
    with pytest.raises(ValueError, match="polygon_iou.*needs polygons=True"):
        driver.TilePipeline(None, 18, polygon_iou=True)
    driver.refuse_polygon_iou_option("X", "why", polygon_iou=False, polygons=True)
    driver.refuse_polygon_iou_option("X", "why")
    with pytest.raises(ValueError, match="ScenePipeline.*polygon_iou is a TilePipeline option"):
        ScenePipeline(None, 18, polygons=True, polygon_iou=True)
    with pytest.raises(ValueError, match="InstancePipeline.*polygon_iou is a TilePipeline option"):
        driver.InstancePipeline(None, 1, prompt="box", polygon_iou=True)
    # one declaration: the table is there with the option and only then
    assert "polygon_counts" not in [t.field for t in driver.output_tables()]
    tab = [t for t in driver.output_tables(polygon_iou=True) if t.field == "polygon_counts"][0]
    assert tab.tail == (3,) and tab.dtype == torch.int64
    assert [t.field for t in driver.output_tables(mask_boxes=True, polygon_iou=True) if t.field != "polygon_counts"] == \
        [t.field for t in driver.output_tables(mask_boxes=True)]
    # the CLIs
    ap = relabel.build_parser()
    assert ap.parse_args(["--ins", "a", "--out", "b"]).masks_from == "rle"
    assert ap.parse_args(["--ins", "a", "--out", "b", "--masks-from", "polygons"]).masks_from == "polygons"
    for bad in (["--masks-from", "mask"], ["--polygon-iou"]):        # an unknown source; the option without polygons
        with pytest.raises(SystemExit):
            ap.parse_args(["--ins", "a", "--out", "b"] + bad)
    assert ap.parse_args(["--ins", "a", "--out", "b", "--polygon-iou", "--polygon-epsilon", "1"]).polygon_iou


def test_tile_result_polygon_iou():
    r = driver.TileResult("k", None, np.zeros(3, np.int64), None, np.zeros(3))
    with pytest.raises(ValueError):
        r.polygon_iou(0)
    r.polygon_counts = np.array([[10, 10, 10], [-1, 4, 0], [6, 8, 4]], np.int64)
    assert r.polygon_iou(0) == 1.0 and r.polygon_iou(1) is None and r.polygon_iou(2) == 0.4


# ---- statistic/polygon_iou.json over two ranks: sets chosen so that the mean, the area ratio and the minimum all differ, and so
# ---- that no rank's own figures are the answer
RANK_COUNTS = [np.array([[100, 100, 100], [10, 20, 5], [-1, 7, 0]], np.int64),          # IoUs 1.0, 0.2, (not traced)
               np.array([[1000, 1200, 900], [4, 4, 3], [0, 0, 0]], np.int64)]           # 900/1300, 0.6, 1.0 (both empty)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    stat = driver.PolygonIoUStat()
    for row in RANK_COUNTS[rank]:                                    # image by image, as the sink adds them
        stat.add(row[None])
    out[rank] = driver.reduce_polygon_iou(stat, 1.5)
    dist.barrier()
    dist.destroy_process_group()


def _serial():
    c = np.concatenate(RANK_COUNTS)
    c = c[c[:, 0] >= 0]
    iou = polygons.iou_from_counts(c)
    union = c[:, 0] + c[:, 1] - c[:, 2]
    return {"n": len(c), "average": float(iou.sum() / len(c)), "area": int(c[:, 2].sum()) / int(union.sum()), "min": float(iou.min()),
            "polygon_epsilon": 1.5}


def test_two_rank_polygon_iou_equals_serial():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    want = _serial()
    assert want["n"] == 5 and want["min"] == 0.2 and len({round(want[k], 9) for k in ("average", "area", "min")}) == 3
    for r in (0, 1):
        got = out[r]
        assert got["n"] == want["n"] and got["min"] == want["min"] and got["area"] == want["area"] and got["polygon_epsilon"] == 1.5
        assert abs(got["average"] - want["average"]) < 1e-15
    one = driver.PolygonIoUStat()
    for row in RANK_COUNTS[0]:
        one.add(row[None])
    alone = driver.reduce_polygon_iou(one, 0.0)                      # no process group: this rank's own figures
    assert alone["n"] == 2 and alone["min"] == 0.2 and alone["average"] == 0.6 and alone["area"] == 105 / 125
    assert alone != {k: want[k] for k in alone}
    empty = driver.reduce_polygon_iou(driver.PolygonIoUStat(), 2.0)
    assert empty == {"n": 0, "average": None, "area": None, "min": None, "polygon_epsilon": 2.0}
