"""No GPU: the host restatement of the polygon tracing (tests/polygon_ref.py) against its own invariants on seeded masks and against
hand-written known answers; samrs_amd/polygons.py (rings_of, nest, coco_segmentation, rasterize); the C ABI declaration and its
ctypes binding; the pickle keys and the flags of the generation CLI."""
import os
import pickle
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_ref  # noqa: E402
import polygon_ref  # noqa: E402

from samrs_amd import polygons  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _seeded_masks():
    """400 masks (some come out empty) no larger than 24 x 24: noise at three densities, rotated bars, disks, disks with stray pixels
    (the recipe of tests/test_mask_boxes_host.py)."""
    rng = np.random.default_rng(20241)
    out = []
    for i in range(400):
        h, w = (int(v) for v in rng.integers(1, 25, 2))
        kind = i % 4
        if kind == 0:
            m = (rng.random((h, w)) < rng.choice([0.02, 0.1, 0.5])).astype(np.uint8)
        elif kind == 1:
            m = box_ref.rotated_bar(24, rng.uniform(0, 180), rng.uniform(3, 20), rng.uniform(1, 6))[:h, :w]
        elif kind == 2:
            m = box_ref.disk(24, rng.uniform(2, 22))[:h, :w]
        else:
            m = box_ref.disk(24, rng.uniform(2, 12))[:h, :w].copy()
            for _ in range(3):
                m[rng.integers(0, h), rng.integers(0, w)] = 1
        out.append(np.ascontiguousarray(m))
    return out


def _rings(mask, x0=0, y0=0):
    v, r, c, t = polygon_ref.mask_polygons([mask], x0, y0)
    return polygons.rings_of(t, r, v, 0), r


def test_invariants_on_seeded_masks():
    checked = 0
    for i, m in enumerate(_seeded_masks()):
        h, w = m.shape
        ids, succ, corner = polygon_ref.edges(m)
        assert ids.size == polygon_ref.count_edges(m)
        assert np.array_equal(np.sort(succ), np.arange(ids.size)), f"mask {i}: the successor is not a bijection"
        x0, y0 = (0, 0) if i % 3 else (7 * i, 3 * i)
        rl, rec = _rings(m, x0, y0)
        if not m.any():
            assert rl == [] and ids.size == 0
            continue
        leader, rank = polygon_ref.walk(ids, succ)
        # the leader is a top edge for a ring of positive area, a bottom edge for a hole; leaders ascend
        assert len(rec) == len(set(leader.tolist())) and np.all(np.diff(rec[:, 3]) >= 0)
        for (pts, hole), r, ld in zip(rl, rec, sorted(set(leader.tolist()))):
            assert int(ids[ld] & 3) == (2 if hole else 0) and int(ids[ld] >> 2) == int(r[3])
            assert (r[2] < 0) == hole and r[2] != 0 and polygons.signed_area2(pts) == int(r[2])
            k = len(pts)
            assert k >= 4 and k % 2 == 0 and k == int(r[1])
            a, b, c = pts, np.roll(pts, -1, axis=0), np.roll(pts, -2, axis=0)
            cross = (b[:, 0] - a[:, 0]) * (c[:, 1] - b[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - b[:, 0])
            assert np.all(cross != 0), f"mask {i}: three consecutive vertices are collinear"
            assert np.all((a[:, 0] == b[:, 0]) != (a[:, 1] == b[:, 1]))        # axis-parallel edges of non-zero length
            if hole:
                x, y = polygons.hole_pixel(pts)
                assert (y - y0) * w + (x - x0) == int(r[3]) and m[y - y0, x - x0]
        assert int(rec[:, 2].sum()) == 2 * int((m != 0).sum())
        assert np.array_equal(polygons.rasterize(rl, h, w, (x0, y0)), (m != 0).astype(np.uint8)), f"mask {i}: rasterize"
        assert sum(1 for r in rl if not r[1]) == polygon_ref.components(m != 0, True)
        assert sum(1 for r in rl if r[1]) == polygon_ref.enclosed_background_components(m)
        nested = polygons.nest(rl)
        assert len(nested) == sum(1 for r in rl if not r[1]) and sum(len(n[1]) for n in nested) == sum(1 for r in rl if r[1])
        checked += 1
    assert checked >= 300


def test_known_answers():
    one = np.zeros((3, 4), np.uint8)
    one[1, 2] = 1
    v, r, n = polygon_ref.trace(one)
    assert n == 4 and v.tolist() == [[2, 1], [3, 1], [3, 2], [2, 2]] and r.tolist() == [[0, 4, 2, 6]]
    blk = np.zeros((4, 5), np.uint8)
    blk[1:3, 1:4] = 1                                             # 2 rows x 3 columns
    v, r, n = polygon_ref.trace(blk, 10, 20)
    assert n == 10 and v.tolist() == [[11, 21], [14, 21], [14, 23], [11, 23]] and r.tolist() == [[0, 4, 12, 6]]
    diag = np.eye(2, dtype=np.uint8)                               # two diagonal pixels: one ring that touches itself at (1, 1)
    v, r, n = polygon_ref.trace(diag)
    assert n == 8 and r.tolist() == [[0, 8, 4, 0]]
    assert v.tolist() == [[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1]]
    anti = np.ascontiguousarray(diag[:, ::-1])
    v, r, n = polygon_ref.trace(anti)
    assert r.tolist() == [[0, 8, 4, 1]] and v.tolist() == [[1, 0], [2, 0], [2, 1], [1, 1], [1, 2], [0, 2], [0, 1], [1, 1]]
    ring = np.ones((3, 3), np.uint8)
    ring[1, 1] = 0
    v, r, n = polygon_ref.trace(ring)
    assert n == 16 and r.tolist() == [[0, 4, 18, 0], [4, 4, -2, 1]]
    assert v.tolist() == [[0, 0], [3, 0], [3, 3], [0, 3], [2, 1], [1, 1], [1, 2], [2, 2]]
    # a hole whose rank-0 edge is no corner: the polygon starts at the first corner behind it
    wide = np.ones((3, 4), np.uint8)
    wide[1, 1:3] = 0
    v, r, n = polygon_ref.trace(wide)
    assert r.tolist() == [[0, 4, 24, 0], [4, 4, -4, 1]] and v[4:].tolist() == [[1, 1], [1, 2], [3, 2], [3, 1]]
    assert polygon_ref.trace(np.zeros((3, 3), np.uint8))[2] == 0


def test_nest_puts_the_island_beside_its_enclosing_ring():
    m = np.zeros((9, 11), np.uint8)
    m[1:8, 1:8] = 1
    m[2:7, 2:7] = 0
    m[4, 4] = 1                                                   # an island inside the hole
    m[0, 10] = 1                                                  # and a stray pixel outside, not touching the frame
    rl, rec = _rings(m, 5, 6)
    assert [r[1] for r in rl] == [False, False, True, False]
    nested = polygons.nest(rl)
    assert [len(n[1]) for n in nested] == [0, 1, 0]
    assert nested[1][0].tolist() == [[6, 7], [13, 7], [13, 14], [6, 14]] and nested[1][1][0].tolist() == [[7, 8], [7, 13], [12, 13], [12, 8]]
    assert nested[2][0].tolist() == [[9, 10], [10, 10], [10, 11], [9, 11]]
    # a hole inside an island inside a hole: the smallest enclosing outer ring is the parent
    m2 = np.ones((11, 11), np.uint8)
    m2[1:10, 1:10] = 0
    m2[3:8, 3:8] = 1
    m2[5, 5] = 0
    nested = polygons.nest(_rings(m2)[0])
    assert [(polygons.signed_area2(o), [polygons.signed_area2(h) for h in hs]) for o, hs in nested] == [(242, [-162]), (50, [-2])]
    with pytest.raises(ValueError):
        polygons.nest([r for r in rl if r[1]])


def test_coco_segmentation_drops_holes_and_says_so():
    ring = np.ones((3, 3), np.uint8)
    ring[1, 1] = 0
    rl, _ = _rings(ring)
    polys, has_holes = polygons.coco_segmentation(rl)
    assert polys == [[0, 0, 3, 0, 3, 3, 0, 3]] and has_holes is True and all(type(c) is int for c in polys[0])
    assert polygons.coco_segmentation(_rings(np.ones((2, 2), np.uint8))[0]) == ([[0, 0, 2, 0, 2, 2, 0, 2]], False)
    assert "drop" in polygons.coco_segmentation.__doc__.lower()


def test_rings_of_reads_the_overflow_and_cap_codes():
    masks = [np.ones((2, 2), np.uint8), np.eye(3, dtype=np.uint8), np.zeros((2, 2), np.uint8)]
    v, r, c, t = polygon_ref.mask_polygons(masks, max_edges=8)
    assert t.tolist() == [[0, 1, 0, 4, 8], [-1, -1, -1, -1, 12], [1, 0, 4, 0, 0]] and c == (4, 1)
    assert polygons.rings_of(t, r, v, 1) is None and polygons.rings_of(t, r, v, 2) == []
    v, r, c, t = polygon_ref.mask_polygons(masks, vertex_capacity=11)
    assert t[1].tolist() == [-1, -2, -1, -13, 12] and polygons.rings_of(t, r, v, 1) is None


def test_reference_is_fast_enough_and_needs_neither_cv2_nor_the_oracle():
    import time
    import region_ref
    m = region_ref.speckled_ellipse(3)
    t0 = time.perf_counter()
    v, r, n = polygon_ref.trace(m)
    dt = time.perf_counter() - t0
    assert 20000 < n < 24000 and int(r[:, 2].sum()) == 2 * int(m.sum())
    assert dt < 5.0, dt                                           # about a second; generous for a loaded machine
    for f in ("polygon_ref.py",):
        assert not re.search(r"^\s*(import|from)\s+(cv2|oracle|torch)", open(os.path.join(ROOT, "tests", f)).read(), flags=re.M)
    assert not re.search(r"^\s*(import|from)\s+(cv2|torch)", open(os.path.join(ROOT, "samrs_amd", "polygons.py")).read(), flags=re.M)


def test_spiral_is_one_ring():
    for n in (13, 96, 130):
        sp = polygon_ref.spiral(n)
        v, r, ne = polygon_ref.trace(sp)
        assert len(r) == 1 and r[0, 1] == len(v) and ne == polygon_ref.count_edges(sp) and ne > n * n       # one ring carries every edge


# ---- the boundary -------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    raw = open(os.path.join(ROOT, "include", "samrs_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    m = re.search(r"int\s+samrs_mask_polygons\s*\(([^)]*)\)\s*;", hdr)
    assert m, "samrs_mask_polygons is not declared in include/samrs_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 15 and params[0].startswith("samrs_engine_t") and params[-1] == "void* stream"
    assert params[7] == "int max_edges" and "int32_t* vertices" in params[8] and "int64_t vertex_capacity" in params[9]
    assert "int32_t* rings" in params[10] and "int64_t ring_capacity" in params[11] and "int64_t* cursor" in params[12]
    assert "int64_t* table" in params[13]
    assert re.search(r"#define\s+SAMRS_ABI_VERSION\s+5\b", raw)
    assert "LATTICE" in raw and "NOT the pixel centres of samrs_mask_boxes" in raw      # the convention differs, and the header says so
    internal = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "samrs_hip_internal.h")).read(), flags=re.S)
    src = open(os.path.join(ROOT, "samrs_amd", "engine.py")).read()
    protos = {"samrs_mask_polygons": m}
    for name in ("samrs_k_polygon_edges", "samrs_k_polygon_ranks"):
        protos[name] = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", internal)
        assert protos[name], name
    for name, proto in protos.items():
        a = re.search(r"lib\." + name + r"\.argtypes\s*=\s*\[([^\]]*)\]", src)
        assert a and len(a.group(1).split(",")) == len(proto.group(1).split(",")), name
    assert "polygon_kernels.hip" in open(os.path.join(ROOT, "samrs_amd", "csrc", "Makefile")).read()
    kernels = open(os.path.join(ROOT, "samrs_amd", "csrc", "polygon_kernels.hip")).read()
    assert "asm" not in re.sub(r"//.*", "", kernels)              # plain C++ only


def test_library_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build_library()
    from samrs_amd import engine
    lib = engine.load_library()
    assert len(lib.samrs_mask_polygons.argtypes) == 15
    assert len(lib.samrs_k_polygon_edges.argtypes) == 11 and len(lib.samrs_k_polygon_ranks.argtypes) == 10
    assert lib.samrs_abi_version() == 5
    assert lib.samrs_k_polygon_edge_stride(10, 10, 65536) == 400 and lib.samrs_k_polygon_edge_stride(1024, 1024, 65536) == 65536
    assert lib.samrs_k_polygon_scratch_bytes(32, 1024, 1024, 65536) <= 256 << 20
    assert lib.samrs_k_polygon_scratch_bytes(1, 10, 10, 3) == -1


# ---- the writers and the flags ------------------------------------------------------------------------------------------------
def test_pickle_keys(tmp_path):
    from samrs_amd import generate
    masks = np.zeros((3, 16, 20), np.uint8)
    masks[0, 2:6, 3:8] = 1
    masks[0, 3, 4] = 0
    masks[1, 8:10, 1:3] = 1
    v, r, c, t = polygon_ref.mask_polygons(list(masks), max_edges=20)
    polys = [polygons.rings_of(t, r, v, j) for j in range(3)]
    assert polys[0] is None and len(polys[1]) == 1 and polys[2] == []
    seg = np.full((16, 20), 255, np.uint8)
    boxes = np.zeros((3, 4), np.float32)
    labels = np.array([1, 0, 2])
    areas = masks.reshape(3, -1).sum(1).astype(np.int64)
    pal = generate.default_palette(3)
    generate.write_outputs(str(tmp_path), "t", seg, masks, boxes, labels, areas, pal, ["a", "b", "c"], polygons=polys)
    info = pickle.load(open(tmp_path / "ins" / "t.pkl", "rb"))
    assert sorted(info[0]) == ["bbox", "category", "label", "mask", "polygon_holes", "polygons", "size"]
    assert info[0]["polygons"] is None and info[0]["polygon_holes"] is None
    assert info[1]["polygon_holes"] == [False] and info[1]["polygons"][0].dtype == np.int32
    assert info[1]["polygons"][0].tolist() == [[1, 8], [3, 8], [3, 10], [1, 10]]
    assert info[2]["polygons"] == [] and info[2]["polygon_holes"] == []
    generate.write_outputs(str(tmp_path / "off"), "t", seg, masks, boxes, labels, areas, pal, ["a", "b", "c"])
    assert sorted(pickle.load(open(tmp_path / "off" / "ins" / "t.pkl", "rb"))[0]) == ["bbox", "category", "label", "mask", "size"]


def test_cli_flags_and_pipeline_arguments():
    import inspect
    from samrs_amd import driver, generate, scene
    base = ["--images", "a", "--boxes", "b", "--out", "c"]
    a = generate.build_parser().parse_args(base)
    assert a.polygons is False and a.polygon_buffer_mb == 64 and a.polygon_max_edges == 65536
    a = generate.build_parser().parse_args(base + ["--polygons", "--polygon-buffer-mb", "8", "--polygon-max-edges", "1000"])
    assert a.polygons is True and a.polygon_buffer_mb == 8 and a.polygon_max_edges == 1000
    for cls in (driver.TilePipeline, scene.ScenePipeline):
        p = inspect.signature(cls.__init__).parameters
        assert p["polygons"].default is False and p["polygon_buffer_mb"].default == 64
    from samrs_amd import engine
    p = inspect.signature(engine.Engine.mask_polygons).parameters
    assert list(p)[1:] == ["masks", "offset", "max_edges", "vertices", "rings", "cursor", "table"] and p["max_edges"].default == 65536
