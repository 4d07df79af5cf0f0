"""CPU: the host side of the mask-quality feature -- samrs_amd/quality.py (stability, inside_fraction, keep_rule), the reference
restatement tests/quality_ref.py on hand-made cases, the C header / ctypes boundary, the generation CLI's flags and what
write_outputs does with the scores."""
import os
import pickle
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref  # noqa: E402

from samrs_amd import quality  # noqa: E402


# ---- quality.py ---------------------------------------------------------------------------------------------------------------
def test_stability_and_inside_fraction_rules():
    c = np.array([[50, 80, 100, 60], [0, 0, 0, 0], [0, 0, 7, 0], [3, 3, 3, 3]], dtype=np.int64)
    s = quality.stability(c)
    assert s.dtype == np.float64 and s.tolist() == [0.5, 0.0, 0.0, 1.0]           # 0 / 0 -> 0.0, not NaN
    f = quality.inside_fraction(c)
    assert f.dtype == np.float64 and f.tolist() == [0.75, 1.0, 1.0, 1.0]          # an empty mask -> 1.0: nothing leaks
    with pytest.raises(ValueError):
        quality.stability(np.zeros((3, 3), np.int64))


def test_keep_rule_compares_fp32_thresholds_in_fp64():
    # 95 / 100 against 0.95: the fp32 threshold is 0.949999988..., and 0.949999988 * 100 <= 95 in fp64 -> kept.  A threshold taken
    # as the DOUBLE 0.95 would give 0.95 * 100 = 94.99999999999999 or 95.00000000000001 depending on rounding; fp32-first is stated.
    c = np.array([[95, 100, 100, 100], [94, 100, 100, 100], [949999989, 10 ** 9, 10 ** 9, 0], [949999988, 10 ** 9, 10 ** 9, 0]], np.int64)
    assert np.float64(np.float32(0.95)) * 1e9 == 949999988.079071
    assert quality.keep_rule(c, None, min_stability=0.95).tolist() == [True, False, True, False]
    # predicted IoU is strict, on fp32 values
    q = np.array([0.88, np.nextafter(np.float32(0.88), np.float32(1)), 0.5, 0.9], dtype=np.float32)
    assert quality.keep_rule(c, q, min_pred_iou=0.88).tolist() == [False, True, False, True]
    with pytest.raises(ValueError):
        quality.keep_rule(c, None, min_pred_iou=0.5)
    with pytest.raises(ValueError):
        quality.keep_rule(c, q[:2], min_pred_iou=0.5)


def test_keep_rule_each_criterion_alone_disabled_and_the_two_library_rules():
    c = np.array([[9, 10, 10, 10],      # stable, inside
                  [1, 10, 10, 10],      # unstable
                  [9, 10, 10, 2],       # leaks out of its box
                  [0, 0, 0, 0],         # empty at every threshold
                  [0, 0, 5, 0]],        # empty mask whose low-threshold mask is not
                 dtype=np.int64)
    q = np.array([0.9, 0.9, 0.9, 0.2, 0.9], dtype=np.float32)
    assert quality.keep_rule(c).all() and quality.keep_rule(c, q, 0, 0, 0).all() and quality.keep_rule(c, q, -1, -1, -1).all()
    assert quality.keep_rule(c, q, min_stability=0.5).tolist() == [True, False, True, False, False]        # 0 / 0 fails
    assert quality.keep_rule(c, q, min_pred_iou=0.5).tolist() == [True, True, True, False, True]
    assert quality.keep_rule(c, q, min_inside_box=0.5).tolist() == [True, True, False, True, True]         # an empty mask passes
    assert quality.keep_rule(c, q, 0.5, 0.5, 0.5).tolist() == [True, False, False, False, False]
    assert quality.keep_rule(np.zeros((0, 4), np.int64)).shape == (0,)


# ---- quality_ref.py -----------------------------------------------------------------------------------------------------------
def test_quality_ref_on_constant_and_hand_made_fields():
    up = quality_ref.logits(torch.full((2, 256, 256), 5.0), (1024, 768), (30, 20))
    assert up.shape == (2, 30, 20) and float((up - 5.0).abs().max()) < 1e-5         # bilinear weights sum to 1, up to rounding
    cnt, band = quality_ref.counts(up, 1.0, [[0, 0, 19, 29], [2.5, 3.5, 4.5, 6.5]])
    assert cnt.tolist() == [[600, 600, 600, 600], [600, 600, 600, 6]] and not band.any()   # x in {3, 4}, y in {4, 5, 6}
    cnt, band = quality_ref.counts(-up, 1.0)
    assert not cnt.any() and quality.stability(cnt).tolist() == [0.0, 0.0]
    assert not quality.keep_rule(cnt, None, min_stability=1e-6).any()
    # a 2 x 2 field: thresholds +-1 and 0, a value exactly on a threshold does not count (strict >), but is in its band
    ref = torch.tensor([[[2.0, 0.5], [-0.5, -1.0]]])
    cnt, band = quality_ref.counts(ref, 1.0, [[1, 0, 1, 1]])
    assert cnt.tolist() == [[1, 2, 3, 1]] and band.tolist() == [[0, 0, 1]]
    assert quality_ref.stability_score(ref, 0.0, 1.0).tolist() == [float(np.float32(1) / np.float32(3))]   # int32 / int32 -> fp32
    assert quality.stability(cnt).tolist() == [1 / 3]
    assert quality_ref.counts(ref, 0.0)[0].tolist() == [[2, 2, 2, 0]]              # offset 0: three equal counts
    # inverted and outside boxes hold nothing; a box over the image holds every set pixel
    m = np.ones((3, 4, 5), np.uint8)
    assert quality_ref.inside_count(m, [[3, 0, 1, 3], [-9, -9, 99, 99], [4.5, 0, 9, 9]]).tolist() == [0, 20, 0]
    assert quality_ref.repaint(m[:2] * np.array([1, 1])[:, None, None], [7, 9], np.array([True, False])).tolist() == [[7] * 5] * 4


def test_quality_ref_identity_shape_reproduces_a_plain_upsample():
    low = quality_ref.make_low(1)
    a = quality_ref.logits(low, (1024, 1024), (1024, 1024))
    b = torch.nn.functional.interpolate(low[None], (1024, 1024), mode="bilinear", align_corners=False)[0]
    assert torch.equal(a, b)                                                      # same-size second stage is the identity
    assert quality_ref.SHAPES[0] == ((1024, 1024), (1024, 1024)) and len(quality_ref.SHAPES) == 5


# ---- the boundary -------------------------------------------------------------------------------------------------------------
def test_header_declares_both_entry_points_and_the_binding_agrees():
    raw = open(os.path.join(ROOT, "include", "samrs_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    src = open(os.path.join(ROOT, "samrs_amd", "engine.py")).read()
    for name, n_params in (("samrs_score_masks", 11), ("samrs_filter_masks", 12)):
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/samrs_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == n_params and params[0].startswith("samrs_engine_t") and params[-1] == "void* stream", params
        a = re.search(r"lib\." + name + r"\.argtypes\s*=\s*\[([^\]]*)\]", src)
        assert a and len(a.group(1).split(",")) == n_params, name
    assert re.search(r"#define\s+SAMRS_ABI_VERSION\s+5\b", raw)                   # entry points are only added
    mk = open(os.path.join(ROOT, "samrs_amd", "csrc", "Makefile")).read()
    assert "quality_kernels.hip" in mk and "postprocess_value.h" in mk


def test_library_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build_library()
    from samrs_amd import engine
    lib = engine.load_library()
    assert len(lib.samrs_score_masks.argtypes) == 11 and len(lib.samrs_filter_masks.argtypes) == 12
    assert lib.samrs_abi_version() == 5
    # a null handle is refused before anything is touched
    assert lib.samrs_score_masks(None, None, 1, 1024, 1024, 8, 8, 1.0, None, None, None) == engine.ERR_BAD_ARG
    assert lib.samrs_filter_masks(None, None, 1, 8, 8, None, None, 0.0, 0.0, 0.0, None, None) == engine.ERR_BAD_ARG


# ---- the flags and the writer --------------------------------------------------------------------------------------------------
BASE = ["--images", "i", "--boxes", "b", "--out", "o"]


def test_generate_flags():
    from samrs_amd import generate
    p = generate.build_parser()
    a = p.parse_args(BASE)
    assert a.quality is False and a.min_stability == 0 and a.min_pred_iou == 0 and a.min_inside_box == 0
    a = p.parse_args(BASE + ["--quality", "--min-stability", "0.9", "--min-pred-iou", "0.8", "--min-inside-box", "0.7"])
    assert a.quality is True and (a.min_stability, a.min_pred_iou, a.min_inside_box) == (0.9, 0.8, 0.7)


@pytest.mark.parametrize("flag", [["--quality"], ["--min-stability", "0.9"], ["--min-pred-iou", "0.8"], ["--min-inside-box", "0.5"]])
def test_generate_refuses_each_flag_with_scene_window(flag, capsys):
    from samrs_amd import generate
    with pytest.raises(SystemExit) as e:
        generate.build_parser().parse_args(BASE + ["--scene-window", "512"] + flag)
    assert e.value.code == 2
    assert flag[0] in capsys.readouterr().err


def test_generate_refuses_a_negative_threshold(capsys):
    from samrs_amd import generate
    with pytest.raises(SystemExit):
        generate.build_parser().parse_args(BASE + ["--min-stability", "-0.1"])
    assert "--min-stability" in capsys.readouterr().err


def test_pipelines_that_do_not_score_refuse_the_options_by_name():
    from samrs_amd import driver
    driver.refuse_quality_options("X", "why", quality=False, min_stability=0.0, png_lut=None)
    with pytest.raises(ValueError, match="min_stability"):
        driver.refuse_quality_options("ScenePipeline", "why", min_stability=0.9)
    with pytest.raises(ValueError, match="quality, min_inside_box"):
        driver.refuse_quality_options("InstancePipeline", "why", quality=True, min_inside_box=0.5)


def test_write_outputs_scores_become_entries_and_dropped_instances_leave(tmp_path):
    from samrs_amd import generate
    seg = np.full((16, 20), 255, np.uint8)
    boxes = np.array([[0, 0, 5, 5], [1, 1, 6, 6], [2, 2, 7, 7]], np.float32)
    labels = np.array([1, 2, 3])
    areas = np.array([10, 0, 30])
    counts = np.array([[8, 10, 10, 9], [0, 0, 4, 0], [20, 30, 40, 30]], np.int64)
    scores = {"pred_iou": np.array([0.9, 0.8, 0.7], np.float32), "stability": quality.stability(counts),
              "inside_box": quality.inside_fraction(counts), "kept": np.array([True, False, True])}
    names = [str(i) for i in range(5)]
    rbs = [np.zeros((4, 2), np.float32), None, np.ones((4, 2), np.float32)]
    generate.write_outputs(str(tmp_path), "a", seg, None, boxes, labels, areas, generate.default_palette(5), names,
                           mask_bboxes=[[0, 0, 1, 1], None, [1, 1, 1, 1]], mask_rboxes=rbs, dota_txt=True, scores=scores)
    info = pickle.load(open(tmp_path / "ins" / "a.pkl", "rb"))
    assert [e["label"] for e in info] == [1, 3]                                   # the dropped instance is absent
    assert all(type(e[k]) is float for e in info for k in ("pred_iou", "stability", "inside_box"))
    assert info[0]["stability"] == 0.8 and info[0]["inside_box"] == 0.9 and info[1]["stability"] == 0.5 and info[1]["inside_box"] == 1.0
    assert info[0]["pred_iou"] == float(np.float32(0.9))
    assert len(open(tmp_path / "rbox" / "a.txt").read().splitlines()) == 2
    generate.write_outputs(str(tmp_path), "b", seg, None, boxes, labels, areas, generate.default_palette(5), names)
    plain = pickle.load(open(tmp_path / "ins" / "b.pkl", "rb"))
    assert len(plain) == 3 and "stability" not in plain[0]
