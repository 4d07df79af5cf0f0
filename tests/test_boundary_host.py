"""CPU: the definition of the boundary band (tests/boundary_ref.py) against its (2 d + 1)^2-window form and scipy.ndimage, the
dilation rule, samrs_amd.coco_ap's accumulation on the reference's min-tables, what the metric is for (it tells apart two predictions
mask AP cannot), the CLI's argument errors and the C boundary of the two new entry points.  Nothing touches a device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_ref as bref  # noqa: E402
import coco_ap_ref as ref  # noqa: E402

from samrs_amd import coco_ap  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("samrs_mask_boundary_bits", "samrs_coco_match_min")


def _disc(h, w, cy, cx, r):
    y, x = np.mgrid[:h, :w]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r * r


def _rect(h, w, y0, x0, hh, ww):
    m = np.zeros((h, w), bool)
    m[y0:y0 + hh, x0:x0 + ww] = True
    return m


def _cases():
    h, w = 41, 57
    hole = _rect(h, w, 8, 10, 25, 30)
    hole[20, 24] = False
    line = np.zeros((h, w), bool)
    line[5:35, 30] = True
    out = {"disc": _disc(h, w, 20, 28, 15), "small disc": _disc(h, w, 10, 40, 4), "hole": hole, "line": line,
           "ones": np.ones((h, w), bool), "empty": np.zeros((h, w), bool)}
    for name, (y0, x0) in {"top-left": (0, 0), "top-right": (0, w - 22), "bottom-left": (h - 18, 0), "bottom-right": (h - 18, w - 22),
                           "top": (0, 15), "bottom": (h - 18, 15), "left": (10, 0), "right": (10, w - 22)}.items():
        out["rect " + name] = _rect(h, w, y0, x0, 18, 22)
    return out


@pytest.mark.parametrize("d", [1, 2, 5])
def test_band_equals_the_window_form(d):
    for name, m in _cases().items():
        assert np.array_equal(bref.band(m, d), bref.band_window(m, d)), (name, d)


@pytest.mark.parametrize("d", [1, 2, 5, 9])
def test_band_equals_scipy_binary_erosion(d):
    ndi = pytest.importorskip("scipy.ndimage")
    for name, m in _cases().items():
        want = m & ~ndi.binary_erosion(m, np.ones((3, 3)), iterations=d, border_value=0)
        assert np.array_equal(bref.band(m, d), want), (name, d)


def test_band_known_answers():
    h, w, d = 41, 57, 5
    frame = np.ones((h, w), bool)
    frame[d:h - d, d:w - d] = False
    assert np.array_equal(bref.band(np.ones((h, w), bool), d), frame)                # all ones: a frame of width d
    assert not bref.band(np.zeros((h, w), bool), d).any()
    line = _cases()["line"]
    assert np.array_equal(bref.band(line, 1), line)                                   # nothing survives one erosion
    hole = _cases()["hole"]
    b = bref.band(hole, 2)
    assert b[18:23, 22:27].sum() == 24 and not b[20, 24]                              # the 5 x 5 around a 1-px hole, minus the hole
    assert np.array_equal(bref.band(np.ones((9, 5), bool), 4), np.ones((9, 5), bool)) # w < 2 d + 1: the band is the mask


def test_boundary_dilation():
    assert [coco_ap.boundary_dilation(h, w) for h, w in ((1024, 1024), (800, 1200), (45, 70), (20, 20))] == [29, 29, 2, 1]
    assert [bref.dilation(h, w) for h, w in ((1024, 1024), (800, 1200), (45, 70), (20, 20))] == [29, 29, 2, 1]
    assert coco_ap.boundary_dilation(1024, 1024, 0.01) == 14 and coco_ap.boundary_dilation(3, 3, 0.001) == 1


def _blobs(rng, n, hw):
    h, w = hw
    return np.stack([_disc(h, w, rng.integers(10, h - 10), rng.integers(10, w - 10), rng.integers(4, 18)) |
                     _rect(h, w, rng.integers(0, h - 12), rng.integers(0, w - 20), rng.integers(3, 12), rng.integers(3, 20))
                     for _ in range(n)])


def test_match_iou_is_the_mask_references_loop():
    """boundary_ref.match_iou restates coco_ap_ref.match_counts with the IoU matrix as an argument: on mask IoU they agree."""
    rng = np.random.default_rng(3)
    for _ in range(4):
        g = _blobs(rng, 6, (64, 80))
        p = np.roll(g, (2, -3), axis=(1, 2))[rng.permutation(6)[:5]]
        s = rng.choice([0.9, 0.8, 0.7], 5).astype(np.float32)
        inter, ad, ag = ref.pair_counts(p, g)
        want = ref.match_counts(inter, ad, ag, s)
        got = bref.match_iou(bref.iou_matrix(inter, ad, ag), ad, ag, s)
        for k in ("order", "match", "dt_ignore", "n_valid"):
            assert np.array_equal(got[k], want[k]), k
        assert got["n_kept"] == want["n_kept"]


def test_accumulate_on_the_references_min_tables():
    rng = np.random.default_rng(11)
    images = []
    for _ in range(5):
        g = _blobs(rng, 5, (72, 96))
        p = np.roll(g, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), axis=(1, 2))
        images.append((p, rng.random(5).astype(np.float32), g))
    want, tables = bref.evaluate(images)
    got = coco_ap.accumulate(tables)
    for k in ref.NAMES:
        assert got[k] == want[k], (k, got[k], want[k])                                # float64 equality: identical integers in
    mask_numbers, _ = ref.evaluate(images)
    assert want["AP"] < mask_numbers["AP"]                                            # the min can only lose matches
    rec = coco_ap.ap_record(got, tables, boundary=True, dilation_ratio=0.02, miou={"average": 0.5, "area": 0.25})
    assert rec["iou"] == "min(mask, boundary)" and rec["dilation_ratio"] == 0.02 and rec["boundary_miou"] == {"average": 0.5, "area": 0.25}
    assert rec["matching"] == "by index" and rec["n_images"] == 5
    plain = coco_ap.ap_record(got, tables)
    assert sorted(plain) == sorted(list(ref.NAMES) + ["n_images", "n_gt", "n_dt", "matching"])        # a mask record gains nothing
    assert "boundary_miou" not in coco_ap.ap_record(got, tables, boundary=True)


def test_boundary_iou_tells_apart_what_mask_iou_cannot():
    """Two predictions of one large disc with EQUAL mask IoU >= 0.9: one shifted, one with a ragged outline.  Mask AP50:95 sees
    the same entries for both; their boundary IoUs differ."""
    h = w = 256
    gt = _disc(h, w, 128, 128, 90)
    shifted = _disc(h, w, 128, 132, 90)
    i0, a0, g0 = (int(v) for v in (np.logical_and(shifted, gt).sum(), shifted.sum(), gt.sum()))
    # ragged: the disc with whole spokes cut out of its rim, grown until it loses exactly as many pixels as the shift lost
    lost = g0 - i0
    y, x = np.mgrid[:h, :w]
    ang = np.arctan2(y - 128, x - 128)
    rim = gt & ~_disc(h, w, 128, 128, 78) & (np.floor(ang / (np.pi / 24)).astype(int) % 2 == 0)
    idx = np.flatnonzero(rim)
    assert len(idx) >= lost
    ragged = gt.copy()
    ragged.reshape(-1)[idx[:lost]] = False
    # equal intersection with equal union would need equal areas: give the ragged one the same surplus outside the disc
    extra = np.flatnonzero(_disc(h, w, 128, 128, 96) & ~gt)[:a0 - i0]
    ragged.reshape(-1)[extra] = True
    i1, a1 = int(np.logical_and(ragged, gt).sum()), int(ragged.sum())
    assert (i1, a1) == (i0, a0)
    mask_iou = i0 / (a0 + g0 - i0)
    assert mask_iou >= 0.9
    tabs = [ref.match_masks(p[None], [0.9], gt[None]) for p in (shifted, ragged)]
    assert np.array_equal(tabs[0]["match"], tabs[1]["match"])
    assert ref.accumulate_tables([tabs[0]]) == ref.accumulate_tables([tabs[1]])
    d = bref.dilation(h, w)
    b_shift, b_rag = bref.boundary_iou(shifted, gt, d), bref.boundary_iou(ragged, gt, d)
    assert b_shift != b_rag and max(b_shift, b_rag) < mask_iou
    nums = [bref.evaluate([(p[None], [0.9], gt[None])])[0]["AP"] for p in (shifted, ragged)]
    assert nums[0] != nums[1]


def test_boundary_miou_helper():
    got = coco_ap.boundary_miou([2, 0, 5], [4, 0, 5], [4, 0, 10])
    assert got["average"] == pytest.approx((2 / 6 + 0.0 + 5 / 10) / 3, abs=0) and got["area"] == 7 / 16
    assert coco_ap.boundary_miou([], [], []) == {"average": 0.0, "area": 0.0}


def test_cli_refuses_boundary_without_ap(capsys):
    from samrs_amd import instances
    base = ["--images", "a", "--annotations", "b", "--out", "c", "--prompt", "box"]
    with pytest.raises(SystemExit) as e:
        instances.parse_args(base + ["--boundary"])
    assert e.value.code == 2 and "--boundary needs --ap" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        instances.parse_args(base + ["--gt-labels", "g", "--ap", "--boundary", "--dilation-ratio", "0"])
    args = instances.parse_args(base + ["--gt-labels", "g", "--ap", "--boundary"])
    assert args.boundary and args.ap and args.dilation_ratio == 0.02
    assert not instances.parse_args(base).boundary


def test_pending_stems_under_boundary(tmp_path):
    import json
    from samrs_amd import instances
    os.makedirs(tmp_path / "parts")
    json.dump({"ap": {}}, open(instances.fragment_path(str(tmp_path), "a"), "w"))
    json.dump({"ap": {}, "boundary_ap": {}}, open(instances.fragment_path(str(tmp_path), "b"), "w"))
    assert instances.pending_stems(str(tmp_path), ["a", "b", "c"], need_ap=True) == ["c"]
    assert instances.pending_stems(str(tmp_path), ["a", "b", "c"], need_ap=True, need_boundary=True) == ["a", "c"]


def test_merge_fragments_writes_boundary_ap_json(tmp_path, capsys):
    """Rank 0's merge from hand-made fragments: boundary_ap.json holds the reference's numbers and the Boundary mIoU over the objects
    miou.json covers; ap.json and miou.json are what a merge without the flag writes."""
    import json
    from samrs_amd import instances, rle
    rng = np.random.default_rng(21)
    out, base = str(tmp_path / "o"), str(tmp_path / "b")
    images, stems = [], ["a", "b"]
    for o in (out, base):
        os.makedirs(os.path.join(o, "parts"))
    for stem, (h, w) in zip(stems, [(72, 96), (60, 81)]):
        g = _blobs(rng, 4, (h, w))
        p = np.roll(g, (2, -1), axis=(1, 2))
        p[3] = g[3] = False                                                           # an object with an empty union: in no mIoU
        s = rng.random(4).astype(np.float32)
        images.append((p, s, g))
        d = bref.dilation(h, w)
        bp, bg = bref.bands(p, d), bref.bands(g, d)
        mask_t, min_t = ref.match_masks(p, s, g), bref.match_masks_min(p, s, g, d)
        min_t.update(band_inter=(bp & bg).sum((1, 2)), band_area_d=bp.sum((1, 2)), band_area_g=bg.sum((1, 2)))
        counts = [rle.encode(m)["counts"] for m in p], [rle.encode(m)["counts"] for m in g]
        common = (h, w, s, counts[0], p.sum((1, 2)), (p & g).sum((1, 2)), g.sum((1, 2)), counts[1])
        instances.write_fragment(out, stem, instances.make_fragment(*common, ap=mask_t, boundary=min_t))
        instances.write_fragment(base, stem, instances.make_fragment(*common, ap=mask_t))
    instances.merge_fragments(base, stems, "rhbox", True, True)
    before = capsys.readouterr().out.splitlines()
    instances.merge_fragments(out, stems, "rhbox", True, True, True, 0.02)
    lines = capsys.readouterr().out.splitlines()
    for name in ("miou.json", "ap.json", "sam_ins_rhbox.json", "gt_ins_rhbox.json"):
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(base, name), "rb").read(), name
    assert not os.path.exists(os.path.join(base, "boundary_ap.json"))
    rec = json.load(open(os.path.join(out, "boundary_ap.json")))
    want, _ = bref.evaluate(images)
    for k in ref.NAMES:
        assert rec[k] == want[k], k
    bands = [(bref.band(p[j], bref.dilation(*p.shape[1:])), bref.band(g[j], bref.dilation(*p.shape[1:]))) for p, _, g in images for j in range(3)]
    assert rec["boundary_miou"]["area"] == sum(int((a & b).sum()) for a, b in bands) / sum(int((a | b).sum()) for a, b in bands)
    per = [bref.boundary_iou(p[j], g[j], bref.dilation(*p.shape[1:])) for p, _, g in images for j in range(3)]
    assert rec["boundary_miou"]["average"] == float(np.mean(per)) and json.load(open(os.path.join(out, "miou.json")))["n_instances"] == 6
    assert rec["iou"] == "min(mask, boundary)" and rec["dilation_ratio"] == 0.02 and rec["matching"] == "by index" and rec["n_dt"] == 8
    assert lines[:len(before)] == before and len(lines) == len(before) + 14
    assert lines[len(before)].startswith("Boundary AP") and lines[len(before) + 1:len(before) + 13] == coco_ap.summary_lines(rec)
    assert lines[-1].startswith("Boundary mIOU")
    with pytest.raises(RuntimeError, match="--boundary"):
        instances.merge_fragments(base, stems, "rhbox", True, True, True)


def test_pipelines_refuse_the_option_by_name():
    from samrs_amd import driver, scene
    for cls in (driver.TilePipeline, scene.ScenePipeline):
        with pytest.raises(ValueError, match="boundary is an InstancePipeline option"):
            cls(None, 1, boundary=True)
    with pytest.raises(ValueError, match="needs ap=True"):
        driver.InstancePipeline(None, 1, gt=True, boundary=True)
    assert [t.field for t in driver.output_tables(gt=True, instance=True, ap=True, boundary=True)][-8:] == [
        "boundary_order", "boundary_match", "boundary_dt_ignore", "boundary_n_valid", "boundary_n_kept", "band_inter", "band_area_d",
        "band_area_g"]
    assert driver.output_tables(gt=True, instance=True, ap=True) == driver.output_tables(gt=True, instance=True, ap=True, boundary=False)


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "samrs_hip.h")).read(), flags=re.S)


def test_the_new_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build_library()
    from samrs_amd import engine
    text = _header()
    lib = engine.load_library()
    raw = ctypes.CDLL(engine.LIB_PATH)
    for name in FUNCTIONS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/samrs_hip.h"
        assert hasattr(raw, name), f"{name} is not exported"
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(m.group(1).split(",")), name
        assert fn.restype is ctypes.c_int
    # samrs_coco_match_min = samrs_coco_match's parameters with the second triple behind the first
    plain = re.search(r"\bint\s+samrs_coco_match\s*\(([^)]*)\)\s*;", text).group(1).split(",")
    both = re.search(r"\bint\s+samrs_coco_match_min\s*\(([^)]*)\)\s*;", text).group(1).split(",")
    norm = lambda ps: [" ".join(p.split()) for p in ps]
    assert norm(both[:4]) == norm(plain[:4]) and norm(both[7:]) == norm(plain[4:])
    assert norm(both[4:7]) == ["const int64_t* inter_b", "const int64_t* area_db", "const int64_t* area_gb"]
    raw.samrs_abi_version.restype = ctypes.c_int
    assert raw.samrs_abi_version() == 5


def test_the_header_states_the_rules():
    text = open(os.path.join(ROOT, "include", "samrs_hip.h")).read()
    for phrase in ("max(1, int(round(ratio * hypot(H, W))))", "M[y][x] AND NOT E[y][x]", "(2 d + 1) x (2 d + 1) square",
                   "min(mask IoU, boundary IoU)", "MASK areas", "must not overlap planes", "stream-ordered"):
        assert phrase in text, phrase
