"""CPU: the overlap rule's host reference on hand-made cases, the C boundary of samrs_resolve_overlaps, and the pure parts of the
``overlap`` option (output_tables, validate_output_options, the pipelines and the CLI that refuse it).  Nothing touches a device."""
import inspect
import os
import pickle
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _masks(*rows):
    return np.array(rows, dtype=np.uint8)[:, None, :]            # [n, 1, W]


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def test_a_tie_goes_to_the_later_mask():
    m = _masks([1, 1, 0, 0], [0, 1, 1, 0], [0, 1, 0, 0])
    out, owner, before, removed = overlap_ref.resolve(m)                              # no logits, no key: everything ties
    assert owner.tolist() == [[0, 2, 1, -1]]
    assert out[:, 0].tolist() == [[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0]]
    assert before.tolist() == [2, 2, 1] and removed.tolist() == [1, 1, 0]
    v = np.zeros((3, 1, 4), np.float32)                                               # equal logits tie too
    assert overlap_ref.resolve(m, v)[1].tolist() == [[0, 2, 1, -1]]
    v[1, 0, 1] = np.nan                                                               # not comparable: the later mask still takes it
    assert overlap_ref.resolve(m, v)[1].tolist() == [[0, 2, 1, -1]]
    v[:, 0, 1] = [0.0, 0.0, np.nan]
    assert overlap_ref.resolve(m, v)[1].tolist() == [[0, 2, 1, -1]]


def test_a_negative_logit_loses_a_contested_pixel_and_wins_an_uncontested_one():
    m = _masks([255, 255, 0], [255, 0, 255])
    v = np.array([[[-3.0, -2.0, 9.0]], [[1.0, 5.0, -4.0]]], np.float32)
    out, owner, before, removed = overlap_ref.resolve(m, v, overlap_ref.primary(m, "logit"))
    assert owner.tolist() == [[1, 0, 1]]            # pixel 0: +1 beats -3; pixel 1: mask 0 alone, at -2; pixel 2: mask 1 alone, at -4
    assert out[:, 0].tolist() == [[0, 255, 0], [255, 0, 255]]                         # winners keep their byte value
    assert removed.tolist() == [1, 0] and before.tolist() == [2, 2]
    v[0, 0, 0] = 2.0                                                                  # now the earlier mask is higher: it keeps the pixel
    assert overlap_ref.resolve(m, v)[1].tolist() == [[0, 0, 1]]


def test_smallest_first_then_the_logit_then_the_index():
    m = _masks([1, 1, 1, 1, 0, 0], [0, 0, 1, 1, 0, 0], [0, 0, 0, 1, 1, 0])
    P = overlap_ref.primary(m, "smallest")
    assert P.tolist() == [-4, -2, -2]
    v = np.zeros((3, 1, 6), np.float32)
    v[1, 0, 3], v[2, 0, 3] = 2.0, 1.0
    assert overlap_ref.resolve(m, v, P)[1].tolist() == [[0, 0, 1, 1, 2, -1]]          # equal areas at pixel 3: the higher logit
    v[2, 0, 3] = 2.0
    assert overlap_ref.resolve(m, v, P)[1].tolist() == [[0, 0, 1, 2, 2, -1]]          # equal logits too: the later mask
    assert overlap_ref.resolve(m, None, P)[1].tolist() == [[0, 0, 1, 2, 2, -1]]       # no logits: the later mask of equal area
    out, _, before, removed = overlap_ref.resolve(m, None, P)
    assert before.tolist() == [4, 2, 2] and removed.tolist() == [2, 1, 0]
    assert ((out != 0).sum(0) <= 1).all() and np.array_equal((out != 0).any(0), (m != 0).any(0))


def test_priority_rule():
    m = _masks([1, 1, 1], [1, 1, 0], [1, 0, 1])
    v = np.array([[[0.0, 0.0, 0.0]], [[9.0, 9.0, 9.0]], [[5.0, 5.0, 5.0]]], np.float32)
    P = overlap_ref.primary(m, "priority", [7, -1, 7])
    assert overlap_ref.resolve(m, v, P)[1].tolist() == [[2, 0, 2]]                    # the key first, whatever the logits say
    assert overlap_ref.resolve(m, None, P)[1].tolist() == [[2, 0, 2]]
    v[2] = -1.0
    assert overlap_ref.resolve(m, v, P)[1].tolist() == [[0, 0, 0]]                    # equal keys: the logit
    with pytest.raises(ValueError):
        overlap_ref.primary(m, "nearest")


def test_band_and_paint_helpers():
    m = _masks([1, 1, 1], [1, 1, 0])
    v = np.array([[[1.0, 1.0, 1.0]], [[1.000001, 3.0, 1.0]]], np.float32)
    assert overlap_ref.band(m, v, 1e-5).tolist() == [[True, False, False]]            # close and contested only
    assert overlap_ref.paint(m, [4, 9]).tolist() == [[9, 9, 4]]
    assert overlap_ref.resolve(np.zeros((0, 2, 2), np.uint8))[1].shape == (0, 0)


# ---- the boundary -------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_point_and_the_binding_agrees():
    raw = open(os.path.join(ROOT, "include", "samrs_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    src = open(os.path.join(ROOT, "samrs_amd", "engine.py")).read()
    m = re.search(r"int\s+samrs_resolve_overlaps\s*\(([^)]*)\)\s*;", hdr)
    assert m, "samrs_resolve_overlaps is not declared in include/samrs_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 14 and params[0].startswith("samrs_engine_t") and params[-1] == "void* stream", params
    a = re.search(r"lib\.samrs_resolve_overlaps\.argtypes\s*=\s*\[([^\]]*)\]", src)
    assert a and len(a.group(1).split(",")) == 14
    e = re.search(r"enum\s+samrs_overlap_rule\s*\{([^}]*)\}", hdr)
    assert e and [s.strip() for s in e.group(1).split(",")] == ["SAMRS_OVERLAP_LOGIT = 1", "SAMRS_OVERLAP_SMALLEST = 2",
                                                               "SAMRS_OVERLAP_PRIORITY = 3"]
    assert re.search(r"#define\s+SAMRS_ABI_VERSION\s+5\b", raw)                   # entry points are only added
    mk = open(os.path.join(ROOT, "samrs_amd", "csrc", "Makefile")).read()
    assert "overlap_kernels.hip" in mk and re.search(r"overlap_kernels\.o[^\n]*:\s*postprocess_value\.h", mk)


def test_library_exports_the_entry_point():
    import __graft_entry__ as ge
    ge.build_library()
    from samrs_amd import engine
    lib = engine.load_library()
    assert len(lib.samrs_resolve_overlaps.argtypes) == 14 and lib.samrs_abi_version() == 5
    assert engine.OVERLAP_RULES == overlap_ref.RULES
    # a null handle is refused before anything is touched
    assert lib.samrs_resolve_overlaps(None, None, 1, 8, 8, 1, None, 1024, 1024, None, None, None, None, None) == engine.ERR_BAD_ARG


# ---- the option ---------------------------------------------------------------------------------------------------------------
def test_output_tables_declare_removed_once():
    import torch
    from samrs_amd import driver
    assert "removed" not in [t.field for t in driver.output_tables()]
    assert [t.field for t in driver.output_tables(overlap="order")] == [t.field for t in driver.output_tables()]
    for rule in ("logit", "smallest"):
        tabs = driver.output_tables(min_region_area=8, mask_boxes=True, overlap=rule)
        hit = [t for t in tabs if t.field == "removed"]
        assert len(hit) == 1 and hit[0].dev == "rem_dev" and hit[0].tail == () and hit[0].dtype == torch.int64
        assert [t.field for t in tabs if t.field != "removed"] == [t.field for t in driver.output_tables(min_region_area=8, mask_boxes=True)]
    assert "removed" in {f.name for f in __import__("dataclasses").fields(driver.TileResult)}
    assert driver.TileResult("k", None, None, None, None).removed is None


def test_validate_output_options_checks_the_value():
    from samrs_amd import driver
    assert driver.OVERLAP_OPTIONS == ("order", "logit", "smallest")
    for v in driver.OVERLAP_OPTIONS:
        assert driver.validate_output_options(overlap=v) == (None, None)
    for bad in ("priority", "Logit", "", None, 1):
        with pytest.raises(ValueError, match="overlap"):
            driver.validate_output_options(overlap=bad)
    assert inspect.signature(driver.TilePipeline.__init__).parameters["overlap"].default == "order"


def test_pipelines_that_do_not_resolve_refuse_the_option_by_name():
    from samrs_amd import driver
    from samrs_amd.scene import ScenePipeline
    driver.refuse_overlap_option("X", "why", overlap="order", quality=True)
    driver.refuse_overlap_option("X", "why")
    with pytest.raises(ValueError, match=r"InstancePipeline.*overlap='logit'"):
        driver.refuse_overlap_option("InstancePipeline", "why", overlap="logit")
    # both constructors refuse before they look at the model
    with pytest.raises(ValueError, match="overlap='smallest'"):
        driver.InstancePipeline(None, 1, overlap="smallest")
    with pytest.raises(ValueError, match=r"ScenePipeline.*overlap='logit'"):
        ScenePipeline(None, 18, window=256, overlap="logit")


BASE = ["--images", "i", "--boxes", "b", "--out", "o"]


def test_generate_flag_and_scene_window(capsys):
    from samrs_amd import generate
    p = generate.build_parser()
    assert p.parse_args(BASE).overlap == "order"
    assert p.parse_args(BASE + ["--overlap", "smallest"]).overlap == "smallest"
    assert p.parse_args(BASE + ["--overlap", "order", "--scene-window", "512"]).overlap == "order"
    for v in ("logit", "smallest"):
        with pytest.raises(SystemExit) as e:
            p.parse_args(BASE + ["--scene-window", "512", "--overlap", v])
        assert e.value.code == 2 and "--overlap" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        p.parse_args(BASE + ["--overlap", "priority"])


def test_write_outputs_removed_becomes_an_entry(tmp_path):
    from samrs_amd import generate
    seg = np.full((16, 20), 255, np.uint8)
    boxes = np.array([[0, 0, 5, 5], [1, 1, 6, 6]], np.float32)
    labels, areas, names = np.array([1, 2]), np.array([10, 7]), [str(i) for i in range(5)]
    generate.write_outputs(str(tmp_path), "a", seg, None, boxes, labels, areas, generate.default_palette(5), names,
                           removed=np.array([0, 3], np.int64))
    info = pickle.load(open(tmp_path / "ins" / "a.pkl", "rb"))
    assert [e["removed"] for e in info] == [0, 3] and all(type(e["removed"]) is int for e in info)
    assert [e["size"] for e in info] == [10, 7]
    generate.write_outputs(str(tmp_path), "b", seg, None, boxes, labels, areas, generate.default_palette(5), names)
    assert "removed" not in pickle.load(open(tmp_path / "ins" / "b.pkl", "rb"))[0]
