"""CPU: the host statement of samrs_simplify_polygons (tests/polygon_simplify_ref.py) on hand-made rings whose answers are worked
out here by hand, the tie rule, ``polygons.rasterize_any`` against ``polygons.rasterize``, the option's validation and what the
headers, the binding and the CLIs declare.  Nothing touches a device."""
import os
import re
import sys

import numpy as np
import pytest

from samrs_amd import driver, polygons

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polygon_ref  # noqa: E402
import polygon_simplify_ref as ps_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kept(pts, eps_q):
    idx, depth = ps_ref.simplify_ring(np.asarray(pts), eps_q)
    assert ps_ref.check_ring(pts, np.asarray(pts)[idx], eps_q)
    return idx, depth


def test_single_pixel():
    sq = [(0, 0), (1, 0), (1, 1), (0, 1)]
    # A = 0, B = 2 (|d|^2 = 2), C: |cross| = 1 at both 1 and 3 -> 1.  Vertex 3 against the segment (1, 1) - (0, 0): N / D = 1 / 2, kept
    # while 256 * 1 > eps_q^2 * 2, i.e. eps_q <= 11
    assert ps_ref.anchors(sq) == (0, 2, 1)
    assert ps_ref.dist_nd((1, 1), (0, 0), (0, 1)) == (1, 2)
    assert _kept(sq, 11) == ([0, 1, 2, 3], 2) and _kept(sq, 12) == ([0, 1, 2], 1) and _kept(sq, 16384)[0] == [0, 1, 2]
    # the offset cannot matter
    assert _kept([(x + 30000, y + 7) for x, y in sq], 12)[0] == [0, 1, 2]


def test_one_by_w_bar():
    bar = [(5, 17), (60, 17), (60, 18), (5, 18)]
    assert ps_ref.anchors(bar) == (0, 2, 1)
    assert ps_ref.dist_nd((60, 18), (5, 17), (5, 18)) == (55 * 55, 55 * 55 + 1)      # just under one pixel
    assert _kept(bar, 15)[0] == [0, 1, 2, 3] and _kept(bar, 16)[0] == [0, 1, 2]


def _staircase(n):
    """the ring of the lower-left staircase triangle of side n: pixels (row y, col x) with x <= y"""
    m = np.tril(np.ones((n, n), np.uint8))
    v, r, _ = polygon_ref.trace(m)
    assert len(r) == 1
    return v


def test_staircase_triangle():
    v = _staircase(8)
    assert v[0].tolist() == [0, 0] and v[16].tolist() == [8, 8] and v[17].tolist() == [0, 8] and len(v) == 18
    # A = 0, B = 16 = (8, 8), C = 17 = (0, 8).  Chain (0, 16) is the staircase under the hypotenuse y = x: the corners (k, k) lie on it,
    # the corners (k + 1, k) all 64 / 128 off (1 / sqrt 2 pixel): a tie, so m* = 1.  It is kept while 256 * 64 > 128 eps_q^2: eps_q <= 11.
    assert ps_ref.anchors([tuple(p) for p in v.tolist()]) == (0, 16, 17)
    assert ps_ref.dist_nd((0, 0), (8, 8), (1, 0)) == ps_ref.dist_nd((0, 0), (8, 8), (8, 7)) == (64, 128)
    assert _kept(v, 12) == ([0, 16, 17], 1)
    # at 11 / 16 vertex 1 = (1, 0) is kept; from it to (8, 8) the chord is (7, 8) and vertex (x, y) is |7 y - 8 (x - 1)| / sqrt(113) off:
    # at most 7 / sqrt(113) = 0.66 pixel (49 * 256 = 12544 <= 121 * 113 = 13673): the rest of the staircase goes
    assert _kept(v, 11) == ([0, 1, 16, 17], 2)
    assert len(_kept(v, 1)[0]) == 18 and len(_kept(v, 16384)[0]) == 3


def test_saddle_ring_and_the_zero_length_chord_branch():
    # two unit pixels that meet at the lattice point (1, 1): one 8-connected ring that visits it twice
    m = np.array([[1, 0], [0, 1]], np.uint8)
    v, r, _ = polygon_ref.trace(m)
    assert len(r) == 1 and v.tolist() == [[0, 0], [1, 0], [1, 1], [2, 1], [2, 2], [1, 2], [1, 1], [0, 1]]
    # A = 0, B = 4, C: |cross| = 2 at 1, 3, 5 and 7 -> 1.  Chain (1, 4): both interior vertices 1 / 5 off: dropped at 8 / 16
    # (256 * 1 <= 64 * 5).  Chain (4, 0): vertices 5 and 7 are 4 / 8 off, the second visit of (1, 1) lies on the chord: 5 is kept
    # (256 * 4 > 64 * 8); behind it 6 and 7 are 1 / 5 off (5) - (0): dropped.
    assert ps_ref.anchors([tuple(p) for p in v.tolist()]) == (0, 4, 1)
    assert _kept(v, 8) == ([0, 1, 4, 5], 2)
    assert _kept(v, 1)[0] == list(range(8))
    # L == 0 (a chain whose two ends are the same lattice point): N = |p - a|^2 over D = 1
    assert ps_ref.dist_nd((1, 1), (1, 1), (2, 2)) == (2, 1) and ps_ref.dist_nd((1, 1), (1, 1), (1, 1)) == (0, 1)
    assert ps_ref.dist_nd((4, 4), (4, 4), (7, 5)) == (10, 1) and ps_ref.dist_nd((4, 4), (4, 4), (6, 3)) == (5, 1)


def test_spike_beyond_the_chords_ends():
    # t <= 0: the vertex projects before a; t >= L: behind b.  The distance is to the END POINT, not to the line.
    a, b = (0, 0), (10, 0)
    assert ps_ref.dist_nd(a, b, (-3, 4)) == (25 * 100, 100)        # t = -30 <= 0: |p - a|^2 L
    assert ps_ref.dist_nd(a, b, (13, 4)) == (25 * 100, 100)        # t = 130 >= L = 100: |p - b|^2 L
    assert ps_ref.dist_nd(a, b, (5, 4)) == (40 * 40, 100)          # inside: cross^2
    assert ps_ref.dist_nd(a, b, (0, 4)) == (16 * 100, 100) and ps_ref.dist_nd(a, b, (10, 4)) == (16 * 100, 100)     # t == 0, t == L
    # A = (0, 0), B = (0, -50), so C is the vertex of greatest |x|: (3, 30).  Vertex 1 = (2, 40) lies BEHIND the end of chain (0, 2):
    # t = 1206 >= L = 909, N / D = |(2, 40) - (3, 30)|^2 = 101 (to the line it would be 3600 / 909 = 3.96).  Vertex 3 = (1, 38) lies
    # BEFORE the start of chain (2, 4): t = -634 <= 0, N / D = |(1, 38) - (3, 30)|^2 = 68 (to the line: 5.28).
    ring = [(0, 0), (2, 40), (3, 30), (1, 38), (0, -50), (-2, -20)]
    assert ps_ref.anchors(ring) == (0, 4, 2)
    assert ps_ref.dist_nd(ring[0], ring[2], ring[1]) == (101 * 909, 909) and ps_ref.dist_nd(ring[2], ring[4], ring[3]) == (68 * 6409, 6409)
    # kept while 256 N > eps_q^2 D: 256 * 101 = 25856 > eps_q^2 up to 160; 256 * 68 = 17408 > eps_q^2 up to 131
    assert {1, 3} <= set(_kept(ring, 131)[0])
    k = _kept(ring, 132)[0]
    assert 1 in k and 3 not in k
    assert 1 in _kept(ring, 160)[0] and 1 not in _kept(ring, 161)[0]


def test_ties_go_to_the_smallest_index():
    sq = [(0, 0), (4, 0), (4, 4), (0, 4)]
    assert ps_ref.anchors(sq) == (0, 2, 1)                                          # C: indices 1 and 3 tie
    diamond = [(0, 0), (2, -2), (4, 0), (2, 2)]
    assert ps_ref.anchors(diamond) == (0, 2, 1)
    # B: two vertices equally far from v[0]
    assert ps_ref.anchors([(0, 0), (5, 0), (3, 4), (0, 5), (-1, 2)])[1] == 1
    # a chain with two equal maxima keeps the first; the second is then judged against the new, shorter chain
    ring = [(0, 0), (2, 3), (6, 3), (8, 0), (4, -20)]
    assert ps_ref.anchors(ring) == (0, 4, 3)
    assert ps_ref.dist_nd(ring[0], ring[3], ring[1]) == ps_ref.dist_nd(ring[0], ring[3], ring[2]) == (24 * 24, 64)      # 3 pixels, both
    assert ps_ref.dist_nd(ring[1], ring[3], ring[2]) == (12 * 12, 45)                                                  # 1.79 pixels
    assert _kept(ring, 40) == ([0, 1, 3, 4], 2)                     # 2.5 pixels: vertex 1 is kept, not 2
    assert _kept(ring, 48)[0] == [0, 3, 4]                          # 3 pixels: 256 * 576 > 2304 * 64 fails, both dropped
    assert _kept(ring, 29)[0] == [0, 1, 3, 4] and _kept(ring, 28)[0] == [0, 1, 2, 3, 4]      # 256 * 144 = 36864 against 45 eps_q^2


def test_fast_statement_equals_the_plain_recursion():
    rng = np.random.default_rng(21)
    rings = []
    for side, p in ((40, 0.55), (64, 0.6), (90, 0.5)):
        v, r, _ = polygon_ref.trace((rng.random((side, side)) < p).astype(np.uint8))
        at = 0
        for rec in r:
            rings.append(v[at:at + int(rec[1])])
            at += int(rec[1])
    yy, xx = np.mgrid[0:128, 0:128]
    v, r, _ = polygon_ref.trace((((yy - 63.5) ** 2 + (xx - 63.5) ** 2) <= 3600).astype(np.uint8))
    rings.append(v)
    rings.append(rng.integers(0, 8192, (300, 2)))                   # arbitrary vertices across the whole coordinate range
    long = [q for q in rings if len(q) > 24]
    assert len(long) >= 10 and max(len(q) for q in long) > 250
    for q in long:
        for eps_q in (1, 8, 16, 40, 300):
            assert ps_ref.simplify_ring_fast(q, eps_q) == ps_ref.simplify_ring(q, eps_q)[0]


def test_buffers_statement_and_checker():
    rng = np.random.default_rng(5)
    masks = (rng.random((3, 20, 24)) < 0.4).astype(np.uint8)
    masks[1] = 0
    v, r, c, t = polygon_ref.mask_polygons(masks, 3, 4)
    t2, r2, v2, c2, depth = ps_ref.simplify_buffers(t, r, v, np.asarray(c), 16)
    assert c2[0] < c[0] and c2[1] == c[1] and depth >= 1
    assert np.array_equal(t2[:, [0, 1, 4]], t[:, [0, 1, 4]]) and np.array_equal(r2[:, 2:], r[:, 2:])
    assert t2[1].tolist() == [t[1, 0], 0, t2[2, 2], 0, 0] and t2[2, 2] == t2[0, 2] + t2[0, 3]
    for j in range(3):
        for (b, hb), (a, ha) in zip(polygons.rings_of(t, r, v, j), polygons.rings_of(t2, r2, v2, j)):
            assert hb == ha and ps_ref.check_ring(b, a, 16)
    ring = polygons.rings_of(t, r, v, 0)[0][0]
    with pytest.raises(AssertionError):
        ps_ref.check_ring(ring, ring[1:4], 16)                     # does not begin with v[0]
    with pytest.raises(AssertionError):
        ps_ref.check_ring(ring, ring[:2], 16)                      # fewer than 3


def test_rasterize_any_equals_rasterize_on_rectilinear_rings():
    rng = np.random.default_rng(9)
    for shape, p, origin in (((17, 23), 0.5, (0, 0)), ((30, 11), 0.2, (100, 7)), ((1, 1), 1.0, (0, 0)), ((12, 12), 0.0, (0, 0))):
        m = (rng.random(shape) < p).astype(np.uint8)
        v, r, _ = polygon_ref.trace(m, *origin)
        rings, at = [], 0
        for rec in r:
            rings.append((v[at:at + int(rec[1])], bool(rec[2] < 0)))
            at += int(rec[1])
        a = polygons.rasterize_any(rings, shape[0], shape[1], origin)
        assert np.array_equal(a, polygons.rasterize(rings, shape[0], shape[1], origin)) and np.array_equal(a, m)
    # arbitrary vertices: a triangle, against the definition evaluated per pixel centre in exact doubled integers
    tri = np.array([[1, 1], [13, 4], [5, 11]], np.int32)
    got = polygons.rasterize_any([(tri, False)], 12, 14)
    want = np.zeros((12, 14), np.uint8)
    p = [tuple(2 * int(c) for c in q) for q in tri]
    for y in range(12):
        for x in range(14):
            cx, cy, n = 2 * x + 1, 2 * y + 1, 0
            for (xa, ya), (xb, yb) in zip(p, p[1:] + p[:1]):
                if min(ya, yb) < cy < max(ya, yb):
                    # crossing at X = xa + (cy - ya) (xb - xa) / (yb - ya) <= cx, multiplied out with the sign of the denominator
                    lhs, den = (cy - ya) * (xb - xa), (yb - ya)
                    n += (lhs <= (cx - xa) * den) if den > 0 else (lhs >= (cx - xa) * den)
            want[y, x] = n & 1
    assert np.array_equal(got, want) and 30 < got.sum() < 60                       # the triangle's area is 54


def test_option_validation():
    v = driver.validate_output_options
    assert driver.polygon_eps_q(0.0, False) == 0 and driver.polygon_eps_q(0.0) == 0
    assert driver.polygon_eps_q(1.0) == 16 and driver.polygon_eps_q(0.5) == 8 and driver.polygon_eps_q(2.53) == 40
    assert driver.polygon_eps_q(1024.0) == 16384 and driver.polygon_eps_q(1 / 16) == 1
    assert v(polygons=True, polygon_epsilon=1.0) == v(polygons=True)               # what it hands back does not change
    with pytest.raises(ValueError, match="needs polygons=True"):
        v(polygon_epsilon=1.0)
    with pytest.raises(ValueError, match=">= 0"):
        v(polygons=True, polygon_epsilon=-0.5)
    with pytest.raises(ValueError, match=">= 0"):
        v(polygons=True, polygon_epsilon=float("nan"))
    with pytest.raises(ValueError, match="16384"):
        v(polygons=True, polygon_epsilon=1024.04)
    with pytest.raises(ValueError, match="rounds to 0"):
        v(polygons=True, polygon_epsilon=0.03)
    with pytest.raises(ValueError, match="polygon_epsilon"):
        driver.InstancePipeline(None, 1, prompt="box", polygon_epsilon=1.0)


def test_clis_take_the_option():
    from samrs_amd import generate, relabel
    a = generate.build_parser().parse_args(["--images", "i", "--boxes", "b", "--out", "o", "--polygon-epsilon", "1.5"])
    assert a.polygon_epsilon == 1.5 and not a.polygons                              # implied in run(), not in the parser
    assert generate.build_parser().parse_args(["--images", "i", "--boxes", "b", "--out", "o"]).polygon_epsilon == 0.0
    b = relabel.build_parser().parse_args(["--ins", "i", "--out", "o", "--polygon-epsilon", "2"])
    assert b.polygon_epsilon == 2.0


def test_write_outputs_adds_the_key(tmp_path):
    import pickle
    from samrs_amd import generate
    seg = np.full((4, 4), 255, np.uint8)
    ring = (np.array([[0, 0], [2, 0], [2, 2]], np.int32), False)
    kw = dict(rles=[{"size": [4, 4], "counts": "0"}], polygons=[[ring]])
    args = (seg, None, np.zeros((1, 4)), np.array([0]), np.array([2]), generate.default_palette(2), ["a", "b"])
    generate.write_outputs(str(tmp_path / "on"), "t", *args, polygon_epsilon=1.5, **kw)
    generate.write_outputs(str(tmp_path / "off"), "t", *args, **kw)
    on = pickle.load(open(tmp_path / "on" / "ins" / "t.pkl", "rb"))[0]
    off = pickle.load(open(tmp_path / "off" / "ins" / "t.pkl", "rb"))[0]
    assert on["polygon_epsilon"] == 1.5 and "polygon_epsilon" not in off and sorted(set(on) - set(off)) == ["polygon_epsilon"]
    assert on["polygon_holes"] == [False] and np.array_equal(on["polygons"][0], ring[0])


def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "samrs_hip.h")).read()
    assert re.search(r"#define\s+SAMRS_ABI_VERSION\s+5\b", hdr)                     # entry points are only added
    assert re.search(r"int samrs_simplify_polygons\(samrs_engine_t\* e, int32_t\* vertices, int32_t\* rings, int64_t\* table[^;]*int n, "
                     r"int eps_q,\s*int64_t\* cursor[^;]*void\* stream\);", hdr)
    for phrase in ("1 <= eps_q <= 16384", "fits in int64", "ties go to the smallest index", "floor(eps_q^2 D / 256)",
                   "ORIGINAL ring's twice-signed area", "pinned against cv2", "Topology is NOT preserved"):
        assert phrase in hdr, phrase
    internal = open(os.path.join(ROOT, "include", "samrs_hip_internal.h")).read()
    assert "samrs_k_polygon_simplify_keep" in internal and "samrs_k_polygon_simplify_scratch_bytes" in internal
    assert "launch_polygon_simplify" in open(os.path.join(ROOT, "samrs_amd", "csrc", "kernels.h")).read()
    assert "polygon_simplify_kernels.hip" in open(os.path.join(ROOT, "samrs_amd", "csrc", "Makefile")).read()
    import __graft_entry__ as ge
    ge.build_library()
    from samrs_amd import engine
    lib = engine.load_library()
    assert len(lib.samrs_simplify_polygons.argtypes) == 8 and len(lib.samrs_k_polygon_simplify_keep.argtypes) == 11
    assert lib.samrs_k_polygon_simplify_scratch_bytes(0, 10, 10) == -1 and lib.samrs_k_polygon_simplify_scratch_bytes(1, -1, 10) == -1
    # 21 bytes per vertex, 36 per ring, 8 per row, each array rounded up to 256
    assert 21 * 1000 + 36 * 100 + 8 * 5 <= lib.samrs_k_polygon_simplify_scratch_bytes(4, 1000, 100) <= 21 * 1000 + 36 * 100 + 8 * 5 + 14 * 256
    assert lib.samrs_abi_version() == 5
    assert engine.Engine.polygon_eps_q(1.0) == 16
    for bad in (0.0, 0.03, 1024.04, -1.0, float("nan")):
        with pytest.raises(ValueError):
            engine.Engine.polygon_eps_q(bad)
