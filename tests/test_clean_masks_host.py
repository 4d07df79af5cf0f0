"""No GPU: the host restatement of the small-region removal (tests/region_ref.py) against hand-written known answers and, where
scipy is importable, against scipy.ndimage.label; the C ABI declaration, its ctypes binding and the flags of the two CLIs."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import region_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def A(rows):
    return np.array([[int(c) for c in r] for r in rows], dtype=np.uint8)


def test_tie_keeps_the_component_that_comes_first_in_row_major_order():
    m = A(["0000000",
           "0110110",      # two 3-pixel islands: the left one starts at (1, 1), the right one at (1, 4)
           "0100010",
           "0000000",
           "0011000"])     # and a 2-pixel island
    out, area, changed = region_ref.clean(m, 10, "islands")
    want = A(["0000000",
              "0110000",
              "0100000",
              "0000000",
              "0000000"])
    assert np.array_equal(out, want) and area == 3 and changed == 5


def test_a_region_of_exactly_min_area_stays():
    m = A(["110001",
           "110001",
           "000001"])                       # a 4-pixel and a 3-pixel island
    assert np.array_equal(region_ref.clean(m, 4, "islands")[0], A(["110000", "110000", "000000"]))
    assert np.array_equal(region_ref.clean(m, 3, "islands")[0], m)
    ring = A(["11111",
              "10011",
              "10011",
              "11111"])                     # a hole of 4 pixels
    assert np.array_equal(region_ref.clean(ring, 4, "holes")[0], ring)
    out, area, changed = region_ref.clean(ring, 5, "holes")
    assert out.all() and area == 20 and changed == 4


def test_all_small_keeps_the_largest():
    m = A(["10100",
           "00100",
           "00001",
           "10001",
           "00001"])                        # areas 1, 2, 3, 1
    out, area, changed = region_ref.clean(m, 100, "islands")
    assert np.array_equal(out, A(["00000", "00000", "00001", "00001", "00001"])) and area == 3 and changed == 4
    # not all small: every small one goes, the exception does not apply
    assert np.array_equal(region_ref.clean(m, 3, "islands")[0], out)
    assert np.array_equal(region_ref.clean(m, 2, "islands")[0], A(["00100", "00100", "00001", "00001", "00001"]))


def test_diagonal_neighbours_are_connected():
    m = A(["1000",
           "0100",
           "0010",
           "0001"])
    assert np.array_equal(region_ref.clean(m, 4, "islands")[0], m)            # one component of 4 pixels
    lab = region_ref.labels(m)
    assert (lab[m == 1] == 0).all() and (lab[m == 0] == -1).all()
    # the two triangles beside the diagonal touch diagonally ((0, 1) and (1, 0)): the complement is ONE component too
    comp = region_ref.labels(m, complement=True)
    assert len(set(comp[m == 0].tolist())) == 1
    anti = A(["01",
              "10"])
    assert np.array_equal(region_ref.clean(anti, 2, "islands")[0], anti)


def test_a_hole_on_the_image_border_is_a_component_like_any_other():
    m = A(["1011",
           "1111",
           "1111",
           "1100"])                         # holes of 1 pixel (top border) and 2 pixels (corner)
    out, area, changed = region_ref.clean(m, 2, "holes")
    assert np.array_equal(out, A(["1111", "1111", "1111", "1100"])) and changed == 1
    assert region_ref.clean(m, 3, "holes")[0].all()


def test_empty_and_full_masks_come_back_unchanged():
    for mode in ("holes", "islands", "both"):
        for t in (1, 7, 10 ** 6):
            z, o = np.zeros((5, 9), np.uint8), np.full((5, 9), 255, np.uint8)
            out, area, changed = region_ref.clean(z, t, mode)
            if mode == "islands" or t <= 45:
                assert not out.any() and area == 0 and changed == 0
            else:                            # the complement of an empty mask is one 45-pixel region: "small" below T
                assert out.all() and changed == 45
            out, area, changed = region_ref.clean(o, t, mode)
            assert out.all() and out.max() == 1 and area == 45 and changed == 0


def test_both_is_holes_then_islands():
    m = A(["000000000",
           "011100010",
           "010100000",
           "011100000"])                    # a ring of 8 with a 1-pixel hole, and a 1-pixel island
    out, area, changed = region_ref.clean(m, 9, "both")       # the filled hole lifts the ring to 9 pixels: it stays
    assert np.array_equal(out, A(["000000000", "011100000", "011100000", "011100000"])) and area == 9 and changed == 2
    # islands alone at the same threshold: both are small, the larger stays, the hole too
    assert np.array_equal(region_ref.clean(m, 9, "islands")[0],
                          A(["000000000", "011100000", "010100000", "011100000"]))


def test_min_area_one_changes_nothing():
    rng = np.random.default_rng(3)
    m = (rng.random((40, 50)) < 0.5).astype(np.uint8)
    for mode in ("holes", "islands", "both"):
        out, area, changed = region_ref.clean(m, 1, mode)
        assert np.array_equal(out, m) and changed == 0 and area == int(m.sum())


def _scipy_clean(mask, t, mode):
    """One pass of the semantics, per pixel, on scipy.ndimage.label with the 3 x 3 structure (scipy numbers the components in
    row-major order of their first pixels, so the first maximum of the sizes is the tie rule)."""
    from scipy import ndimage
    mask = mask.astype(bool)
    holes = mode == "holes"
    work = ~mask if holes else mask
    lab, n = ndimage.label(work, structure=np.ones((3, 3), int))
    if n == 0:
        return mask
    sizes = np.bincount(lab.ravel(), minlength=n + 1)
    small = sizes < t
    small[0] = False                                         # label 0 = outside the working set
    if holes:
        return mask | small[lab]
    if not small[1:].any():
        return mask
    if small[1:].all():
        return lab == 1 + int(np.argmax(sizes[1:]))
    return mask & ~small[lab]


def test_reference_against_scipy_label():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(11)
    n_changed = 0
    for k in range(200):
        h, w = int(rng.integers(1, 48)), int(rng.integers(1, 48))
        m = rng.random((h, w)) < rng.choice([0.2, 0.45, 0.6, 0.85])
        if k % 3 == 0:
            m = ndimage.binary_opening(m, iterations=1)
        t = int(rng.choice([1, 2, 3, 5, 9, 30, 5000]))
        lab_ref, _ = ndimage.label(m, structure=np.ones((3, 3), int))
        lab = region_ref.labels(m)
        for v in np.unique(lab_ref[m]):                      # same partition, roots = first pixel
            sel = lab_ref == v
            assert len(np.unique(lab[sel])) == 1 and lab[sel][0] == np.flatnonzero(sel.ravel())[0]
        for mode in ("holes", "islands"):
            got = region_ref.clean(m, t, mode)[0].astype(bool)
            assert np.array_equal(got, _scipy_clean(m, t, mode)), (k, mode, t)
            n_changed += int((got != m).any())
        both = _scipy_clean(_scipy_clean(m, t, "holes"), t, "islands")
        assert np.array_equal(region_ref.clean(m, t, "both")[0].astype(bool), both)
    assert n_changed > 50


def test_header_declares_the_entry_point_and_the_enum():
    hdr = open(os.path.join(ROOT, "include", "samrs_hip.h")).read()
    m = re.search(r"int\s+samrs_clean_masks\s*\(([^)]*)\)\s*;", hdr)
    assert m, "samrs_clean_masks is not declared in include/samrs_hip.h"
    assert len(m.group(1).split(",")) == 10
    e = re.search(r"enum\s+samrs_region_mode\s*\{([^}]*)\}", hdr)
    assert e
    vals = dict((k.strip(), int(v)) for k, v in (kv.split("=") for kv in e.group(1).split(",")))
    assert vals == {"SAMRS_REGION_HOLES": 1, "SAMRS_REGION_ISLANDS": 2, "SAMRS_REGION_BOTH": 3}
    assert re.search(r"#define\s+SAMRS_ABI_VERSION\s+5\b", hdr)
    internal = open(os.path.join(ROOT, "include", "samrs_hip_internal.h")).read()
    assert re.search(r"int\s+samrs_k_region_labels\s*\(", internal)
    # the binding names ten argument types (a library that is not built is no reason to skip: read the source)
    src = open(os.path.join(ROOT, "samrs_amd", "engine.py")).read()
    a = re.search(r"lib\.samrs_clean_masks\.argtypes\s*=\s*\[([^\]]*)\]", src)
    assert a and len(a.group(1).split(",")) == 10
    k = re.search(r"lib\.samrs_k_region_labels\.argtypes\s*=\s*\[([^\]]*)\]", src)
    assert k and len(k.group(1).split(",")) == 7
    from samrs_amd import engine
    assert engine.REGION_MODES == {"holes": 1, "islands": 2, "both": 3}
    if os.path.exists(engine.LIB_PATH):
        lib = engine.load_library()
        assert len(lib.samrs_clean_masks.argtypes) == 10 and len(lib.samrs_k_region_labels.argtypes) == 7


def test_both_command_lines_take_the_flags():
    from samrs_amd import generate, instances
    g = generate.build_parser()
    base = ["--images", "i", "--boxes", "b", "--out", "o"]
    a = g.parse_args(base)
    assert a.min_region_area == 0 and a.region_mode == "both"
    a = g.parse_args(base + ["--min-region-area", "16", "--region-mode", "islands"])
    assert a.min_region_area == 16 and a.region_mode == "islands"
    with pytest.raises(SystemExit):
        g.parse_args(base + ["--region-mode", "speckle"])
    assert "processed in this run" in " ".join(g.format_help().split())
    p = instances.build_parser()
    base = ["--images", "i", "--annotations", "x", "--out", "o", "--prompt", "box"]
    a = p.parse_args(base)
    assert a.min_region_area == 0 and a.region_mode == "both"
    a = p.parse_args(base + ["--min-region-area", "9", "--region-mode", "holes"])
    assert a.min_region_area == 9 and a.region_mode == "holes"
