"""CPU: samrs_amd.coco_ap.accumulate against the sequential reference (tests/coco_ap_ref.py) on random match tables, analytic known
answers that pin both to COCO's definition, and the C boundary of the four entry points.  Nothing touches a device."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coco_ap_ref as ref  # noqa: E402

from samrs_amd import coco_ap  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("samrs_mask_pack_bits", "samrs_label_pack_bits", "samrs_mask_pair_counts", "samrs_coco_match")


def _disc(h, w, cy, cx, r):
    y, x = np.mgrid[:h, :w]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r * r


def _rect(h, w, y0, x0, hh, ww):
    m = np.zeros((h, w), bool)
    m[y0:y0 + hh, x0:x0 + ww] = True
    return m


def _both(images):
    """The twelve numbers from the reference (masks in) and from coco_ap.accumulate on the reference's tables; they must agree."""
    want, tables = ref.evaluate(images)
    got = coco_ap.accumulate(tables)
    assert set(got) == set(ref.NAMES) == set(coco_ap.NAMES)
    for k in ref.NAMES:
        assert got[k] == pytest.approx(want[k], abs=1e-12), (k, got[k], want[k])
    return got


def test_constants_are_cocos():
    assert np.array_equal(coco_ap.IOU_THRESHOLDS, np.linspace(.5, .95, 10))
    assert coco_ap.AREA_RANGES.tolist() == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]
    assert tuple(coco_ap.MAX_DETS) == (1, 10, 100) and len(coco_ap.RECALL_THRESHOLDS) == 101
    assert np.array_equal(ref.THRESHOLDS, coco_ap.IOU_THRESHOLDS)


def test_reference_packing_forms_agree():
    rng = np.random.default_rng(0)
    m = rng.integers(0, 2, (3, 7, 13)).astype(np.uint8) * 255
    a, b = ref.pack_bits(m), ref.pack_bits_fast(m)
    assert a.dtype == np.uint64 and a.shape == (3, 2) and np.array_equal(a, b)
    assert int(a[0, 0]) & 1 == int(m[0, 0, 0] != 0) and not np.any(a[:, 1] >> np.uint64(7 * 13 - 64))      # tail bits zero


@pytest.mark.parametrize("seed", range(6))
def test_accumulate_matches_the_reference_on_random_tables(seed):
    rng = np.random.default_rng(seed)
    A, T, M = 4, 10, 100
    tables = []
    for _ in range(int(rng.integers(1, 7))):
        nd, ng = int(rng.integers(0, 140)), int(rng.integers(0, 9))
        scores = np.round(rng.random(nd), 1).astype(np.float32)                 # many equal scores: the stable sort matters
        order = np.argsort(-scores, kind="mergesort")[:M]
        k = len(order)
        match = -np.ones((A, T, M), np.int32)
        ign = np.zeros((A, T, M), np.uint8)
        if ng and k:
            match[:, :, :k] = rng.integers(-1, ng, (A, T, k))
        ign[:, :, :k] = rng.random((A, T, k)) < 0.2
        n_valid = np.array([ng] + [int(rng.integers(0, ng + 1)) for _ in range(A - 1)], np.int32)
        if seed == 3:
            n_valid[1] = 0                                                      # one range without valid ground truth anywhere
        tables.append({"scores": scores.astype(np.float64), "order": order.astype(np.int32), "match": match, "dt_ignore": ign,
                       "n_valid": n_valid, "n_kept": k})
    want, got = ref.accumulate_tables(tables), coco_ap.accumulate(tables)
    for k in ref.NAMES:
        assert got[k] == pytest.approx(want[k], abs=1e-12), (k, got[k], want[k])
    if seed == 3:
        assert got["APs"] == -1 and got["ARs"] == -1


def test_all_predictions_perfect():
    """Small (r = 5: 81 px), medium (40 x 40) and large (100 x 100) ground truths, each predicted exactly: every populated entry is 1."""
    h = w = 160
    gts = np.stack([_disc(h, w, 10, 10, 5), _rect(h, w, 30, 5, 40, 40), _rect(h, w, 50, 55, 100, 100)])
    got = _both([(gts.copy(), [0.9, 0.8, 0.7], gts), (gts[:2].copy(), [0.5, 0.6], gts[:2])])
    for k in ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR@10", "AR@100", "ARs", "ARm", "ARl"):
        assert got[k] == pytest.approx(1.0, abs=1e-12), k
    assert got["AR@1"] == pytest.approx(2 / 5, abs=1e-12)                    # one detection per image, five ground truths


def test_two_ground_truths_one_perfect_detection():
    """Recall reaches 0.5 with precision 1: the 51 recall levels 0.00 .. 0.50 sample 1, the 50 above sample 0."""
    h = w = 64
    gts = np.stack([_rect(h, w, 2, 2, 10, 10), _rect(h, w, 30, 30, 12, 12)])
    got = _both([(gts[:1].copy(), [0.9], gts)])
    assert got["AP"] == pytest.approx(51 / 101, abs=1e-12) and got["AP50"] == pytest.approx(51 / 101, abs=1e-12)
    assert got["AR@100"] == pytest.approx(0.5, abs=1e-12) and got["AR@1"] == pytest.approx(0.5, abs=1e-12)


def test_ground_truth_without_detections():
    gts = np.stack([_rect(64, 64, 2, 2, 10, 10)])
    got = _both([(np.zeros((0, 64, 64), bool), [], gts)])
    assert got["AP"] == 0 and got["AP50"] == 0 and got["AR@100"] == 0
    assert got["APs"] == 0 and got["APm"] == -1 and got["APl"] == -1


def test_no_ground_truth_in_the_small_range():
    gts = np.stack([_rect(128, 128, 2, 2, 40, 40)])                            # 1600 px: medium
    got = _both([(gts.copy(), [0.9], gts)])
    assert got["APs"] == -1 and got["ARs"] == -1 and got["APl"] == -1 and got["ARl"] == -1
    assert got["APm"] == pytest.approx(1.0, abs=1e-12) and got["AP"] == pytest.approx(1.0, abs=1e-12)


def test_true_false_true():
    """Two ground truths; by score: a true positive (0.9), a false positive (0.8), a true positive (0.7).
    tp = 1, 1, 2 and fp = 0, 1, 1: recall = 0.5, 0.5, 1 and precision = 1, 1/2, 2/3, non-increasing from the right: 1, 2/3, 2/3.
    The recall levels 0.00 .. 0.50 (51 of them) first reach their recall at index 0 and sample 1; the levels 0.51 .. 1.00 (50) at
    index 2 and sample 2/3.  AP = (51 + 50 * 2/3) / 101 = 0.834983..., the same at every threshold (the matches are exact);
    AR@100 = 1, AR@1 = 0.5."""
    h = w = 64
    gts = np.stack([_rect(h, w, 2, 2, 10, 10), _rect(h, w, 30, 30, 12, 12)])
    fp = _rect(h, w, 50, 2, 8, 8)
    got = _both([(np.stack([gts[1], fp, gts[0]]), [0.9, 0.8, 0.7], gts)])
    want = (51 + 50 * (2 / 3)) / 101
    assert got["AP"] == pytest.approx(want, abs=1e-12) and got["AP75"] == pytest.approx(want, abs=1e-12)
    assert got["AR@100"] == pytest.approx(1.0, abs=1e-12) and got["AR@1"] == pytest.approx(0.5, abs=1e-12)


def test_a_match_to_ground_truth_index_0_is_a_true_positive():
    """pycocotools tests the stored annotation id for truth and would lose this match; here a match is a match by index."""
    gts = np.stack([_rect(64, 64, 2, 2, 10, 10)])
    tables = ref.evaluate([(gts.copy(), [0.9], gts)])[1]
    assert tables[0]["match"][0, :, 0].tolist() == [0] * 10 and tables[0]["dt_ignore"][0, :, 0].tolist() == [0] * 10
    got = coco_ap.accumulate(tables)
    assert got["AP"] == pytest.approx(1.0, abs=1e-12) and got["AR@1"] == pytest.approx(1.0, abs=1e-12)
    rec = coco_ap.ap_record(got, tables)
    assert rec["matching"] == "by index" and rec["n_images"] == 1 and rec["n_gt"] == 1 and rec["n_dt"] == 1
    assert "by index" in coco_ap.__doc__.lower() or "BY INDEX" in coco_ap.__doc__


def test_reference_matching_rules():
    """3/5 is below 0.6000000000000001 (what ``linspace(.5, .95, 10)[2]`` was before numpy computed it as exactly 0.6) and not
    below 0.6; equal IoUs go to the later ground truth; equal scores keep index order."""
    inter, ad, ag = np.array([[6]]), np.array([8]), np.array([8])            # IoU 6 / 10
    thr = ref.THRESHOLDS.copy()
    thr[2] = 0.6000000000000001
    t = ref.match_counts(inter, ad, ag, [0.5], thresholds=thr)
    assert t["match"][0, :, 0].tolist() == [0, 0] + [-1] * 8
    t = ref.match_counts(inter, ad, ag, [0.5], thresholds=[0.6])
    assert t["match"][0, :, 0].tolist() == [0]
    t = ref.match_counts(np.array([[8, 8]]), np.array([8]), np.array([8, 8]), [0.5])
    assert t["match"][0, 0, 0] == 1
    t = ref.match_counts(np.zeros((3, 0), int), np.array([5, 5, 5]), np.zeros(0, int), [0.5, 0.7, 0.5])
    assert t["order"].tolist() == [1, 0, 2]


def test_summary_lines_use_cocos_wording():
    numbers = {k: 0.5 for k in coco_ap.NAMES}
    lines = coco_ap.summary_lines(numbers)
    assert len(lines) == 12
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.500"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.500"
    assert lines[11] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = 0.500"


# ---- the C boundary ---------------------------------------------------------------------------------------------------------------
def _prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "samrs_hip.h")).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(samrs_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}, text


def test_header_declares_the_four_functions_at_abi_5():
    protos, text = _prototypes()
    for name in FUNCTIONS:
        assert name in protos, name
    assert re.search(r"#define\s+SAMRS_ABI_VERSION\s+5\b", text)
    from samrs_amd import engine
    assert engine.ABI_VERSION == 5


def test_argtypes_match_the_prototypes():
    import __graft_entry__ as ge
    ge.build_library()
    from samrs_amd import engine
    lib = engine.load_library()
    protos, _ = _prototypes()
    for name in FUNCTIONS:
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(protos[name].split(",")), name
    for name in ("pack_mask_bits", "pack_label_bits", "mask_pair_counts", "coco_match"):
        assert callable(getattr(engine.Engine, name))


def test_ap_option_is_declared_once():
    from samrs_amd import driver
    off = [t.field for t in driver.output_tables(gt=True, rle=True, instance=True)]
    on = [t.field for t in driver.output_tables(gt=True, rle=True, instance=True, ap=True)]
    assert on[:len(off)] == off and set(on) - set(off) == {"ap_order", "ap_match", "ap_dt_ignore", "ap_n_valid", "ap_n_kept"}
    assert driver.TileResult("k", None, None, None, None).ap_tables is None


def test_resume_counts_a_fragment_without_ap_as_not_done(tmp_path):
    import json
    from samrs_amd import instances
    os.makedirs(tmp_path / "parts")
    (tmp_path / "parts" / "a.json").write_text(json.dumps({"height": 1, "width": 1, "scores": [], "rles": []}))
    (tmp_path / "parts" / "b.json").write_text(json.dumps({"height": 1, "width": 1, "scores": [], "rles": [], "ap": {}}))
    assert instances.pending_stems(str(tmp_path), ["a", "b", "c"]) == ["c"]
    assert instances.pending_stems(str(tmp_path), ["a", "b", "c"], need_ap=True) == ["a", "c"]
