"""No GPU: the host restatement of the mask-derived boxes (tests/box_ref.py) against brute force and hand-written known answers;
the C ABI declaration and its ctypes binding; the pickle keys, the DOTA line format, the COCO bbox and the flags of the two CLIs."""
import os
import pickle
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _seeded_masks():
    """320 masks (some come out empty) no larger than 24 x 24: noise at three densities, rotated bars, disks, disks with stray pixels."""
    rng = np.random.default_rng(20240)
    out = []
    for i in range(320):
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


def _points(m, x0=0, y0=0):
    ys, xs = np.nonzero(m)
    return [(x0 + int(x), y0 + int(y)) for x, y in zip(xs, ys)]


def test_hull_and_winning_area_against_brute_force():
    checked = 0
    for i, m in enumerate(_seeded_masks()):
        x0, y0 = (0, 0) if i % 3 else (17 * i, 5 * i)
        pts = _points(m, x0, y0)
        v = box_ref.hull(m, x0, y0)
        if not pts:
            assert v == [] and box_ref.record(v) == (0,) * 8
            continue
        assert v == box_ref.in_definition_order(box_ref.monotone_chain_hull(pts)), f"mask {i}: hull"
        assert v[0] == min(pts, key=lambda p: (p[1], p[0]))
        rec = box_ref.record(v)
        dx, dy, pmin, pmax, qmin, qmax, mm, area2 = rec
        assert mm == len(v) and (pmin, pmax, qmin, qmax) == box_ref.candidate(v, dx, dy)
        assert Fraction((pmax - pmin) * (qmax - qmin), dx * dx + dy * dy) == box_ref.min_area_all_pairs(pts), f"mask {i}: area"
        # every pixel lies inside the rectangle, and the hull's area is the shoelace sum of the brute-force hull
        assert (pmin, pmax, qmin, qmax) == box_ref.candidate(pts, dx, dy)
        ccw = box_ref.monotone_chain_hull(pts)
        assert area2 == sum(ccw[k][0] * ccw[(k + 1) % len(ccw)][1] - ccw[(k + 1) % len(ccw)][0] * ccw[k][1] for k in range(len(ccw)))
        hb = box_ref.hbox(m, x0, y0)
        assert hb == (min(p[0] for p in pts), min(p[1] for p in pts), max(p[0] for p in pts), max(p[1] for p in pts))
        checked += 1
    assert checked >= 200


def test_known_answers():
    m = np.zeros((9, 12), np.uint8)
    m[2:6, 3:8] = 1                                           # 5 x 4 block at columns 3..7, rows 2..5
    hb, rb, rec = box_ref.mask_boxes(m[None])
    assert rec[0].tolist() == [0, 3, 6, 15, -21, -9, 4, 24] and hb[0].tolist() == [3, 2, 7, 5]
    assert rb[0].tolist() == [[7, 2], [7, 5], [3, 5], [3, 2]] and rb.dtype == np.float32
    one = np.zeros((7, 7), np.uint8)
    one[4, 2] = 1
    hb, rb, rec = box_ref.mask_boxes(one[None], 10, 20)
    assert rec[0].tolist() == [1, 0, 12, 12, 24, 24, 1, 0] and hb[0].tolist() == [12, 24, 12, 24]
    assert rb[0].tolist() == [[12, 24]] * 4
    row = np.zeros((5, 9), np.uint8)
    row[3, 2:8] = 1
    row[3, 4] = 0                                             # a gap changes nothing
    hb, rb, rec = box_ref.mask_boxes(row[None])
    assert box_ref.hull(row) == [(2, 3), (7, 3)]
    assert rec[0].tolist() == [5, 0, 10, 35, 15, 15, 2, 0] and rb[0].tolist() == [[2, 3], [7, 3], [7, 3], [2, 3]]
    diag = np.eye(6, dtype=np.uint8)
    hb, rb, rec = box_ref.mask_boxes(diag[None])
    assert box_ref.hull(diag) == [(0, 0), (5, 5)]
    assert rec[0].tolist() == [5, 5, 0, 50, 0, 0, 2, 0] and rb[0].tolist() == [[0, 0], [5, 5], [5, 5], [0, 0]]
    anti = np.ascontiguousarray(np.eye(6, dtype=np.uint8)[:, ::-1])
    assert box_ref.hull(anti) == [(5, 0), (0, 5)]
    d = box_ref.diamond(21, 6)                                 # |dx| + |dy| <= 6 around (10, 10): four equal rectangles, edge 0 wins
    v = box_ref.hull(d)
    assert v == [(10, 4), (4, 10), (10, 16), (16, 10)]
    hb, rb, rec = box_ref.mask_boxes(d[None])
    assert rec[0].tolist() == [-6, 6, -36, 36, -156, -84, 4, 144]
    assert rb[0].tolist() == [[16, 10], [10, 16], [4, 10], [10, 4]]
    hb, rb, rec = box_ref.mask_boxes(np.zeros((2, 4, 4), np.uint8))
    assert not hb.any() and not rb.any() and not rec.any()
    ext = box_ref.row_extents(row)
    assert ext.tolist() == [[-1, -1, 0]] * 3 + [[2, 7, 5], [-1, -1, 0]]


def test_corners_are_one_double_division_rounded_to_float():
    rec = (3, 7, -11, 100, -5, 64, 5, 0)
    L = 58
    want = [[np.float32(np.float64(p * 3 - q * 7) / np.float64(L)), np.float32(np.float64(p * 7 + q * 3) / np.float64(L))]
            for p, q in ((-11, -5), (100, -5), (100, 64), (-11, 64))]
    got = box_ref.corners(rec)
    assert got.dtype == np.float32 and got.tobytes() == np.array(want, dtype=np.float32).tobytes()


def test_box_ref_needs_neither_cv2_nor_the_oracle():
    src = open(os.path.join(ROOT, "tests", "box_ref.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(cv2|oracle)", src, flags=re.M)


# ---- the boundary -------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "samrs_hip.h")).read(), flags=re.S)
    m = re.search(r"int\s+samrs_mask_boxes\s*\(([^)]*)\)\s*;", hdr)
    assert m, "samrs_mask_boxes is not declared in include/samrs_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 11 and params[0].startswith("samrs_engine_t") and params[-1] == "void* stream"
    assert "int32_t* hbox_out" in params[7] and "float* rbox_out" in params[8] and "int64_t* record_out" in params[9]
    assert re.search(r"#define\s+SAMRS_ABI_VERSION\s+5\b", open(os.path.join(ROOT, "include", "samrs_hip.h")).read())
    internal = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "samrs_hip_internal.h")).read(), flags=re.S)
    ke = re.search(r"int\s+samrs_k_mask_row_extents\s*\(([^)]*)\)\s*;", internal)
    kh = re.search(r"int\s+samrs_k_mask_hull\s*\(([^)]*)\)\s*;", internal)
    assert ke and kh
    src = open(os.path.join(ROOT, "samrs_amd", "engine.py")).read()
    for name, proto in (("samrs_mask_boxes", m), ("samrs_k_mask_row_extents", ke), ("samrs_k_mask_hull", kh)):
        a = re.search(r"lib\." + name + r"\.argtypes\s*=\s*\[([^\]]*)\]", src)
        assert a and len(a.group(1).split(",")) == len(proto.group(1).split(",")), name
    assert "box_kernels.hip" in open(os.path.join(ROOT, "samrs_amd", "csrc", "Makefile")).read()
    flags = open(os.path.join(ROOT, "samrs_amd", "csrc", "Makefile")).read()
    assert "fast-math" not in flags and "-mno-" not in flags          # the corner division must stay IEEE


def test_library_exports_the_entry_points():
    import __graft_entry__ as ge
    ge.build_library()
    from samrs_amd import engine
    lib = engine.load_library()
    assert len(lib.samrs_mask_boxes.argtypes) == 11
    assert len(lib.samrs_k_mask_row_extents.argtypes) == 6 and len(lib.samrs_k_mask_hull.argtypes) == 11
    assert lib.samrs_abi_version() == 5


# ---- the writers and the flags ------------------------------------------------------------------------------------------------
def _result(n=3):
    from samrs_amd import driver
    masks = np.zeros((n, 16, 20), np.uint8)
    masks[0, 2:6, 3:8] = 1
    masks[1] = box_ref.rotated_bar(20, 30, 12, 4)[:16]
    hb, rb, rec = box_ref.mask_boxes(masks)
    r = driver.TileResult("t", None, masks.reshape(n, -1).sum(1).astype(np.int64), np.zeros((n, 4), np.float32), np.array([1, 0, 2][:n]))
    r.mask_hbox, r.mask_rbox, r.mask_record = hb, rb, rec
    return r, masks


def test_tile_result_mask_bbox_is_coco_in_whole_pixels():
    r, _ = _result()
    assert r.mask_bbox(0) == [3, 2, 5, 4]
    x, y, w, h = r.mask_bbox(1)
    assert (x, y, x + w - 1, y + h - 1) == tuple(int(v) for v in r.mask_hbox[1])
    assert r.mask_bbox(2) is None                              # an empty mask


def test_pickle_keys_and_dota_lines(tmp_path):
    from samrs_amd import generate
    r, masks = _result()
    names = ["plane", "ship", "bridge"]
    bbs = [r.mask_bbox(j) for j in range(3)]
    rbs = [None if b is None else r.mask_rbox[j] for j, b in enumerate(bbs)]
    seg = np.full((16, 20), 255, np.uint8)
    pal = generate.default_palette(3)
    generate.write_outputs(str(tmp_path), "t", seg, masks, r.boxes, r.labels, r.areas, pal, names, mask_bboxes=bbs, mask_rboxes=rbs,
                           dota_txt=True)
    info = pickle.load(open(tmp_path / "ins" / "t.pkl", "rb"))
    assert sorted(info[0]) == ["bbox", "category", "label", "mask", "mask_bbox", "mask_rbox", "size"]
    assert info[0]["mask_bbox"] == [3, 2, 5, 4] and info[0]["mask_rbox"].dtype == np.float32 and info[0]["mask_rbox"].shape == (4, 2)
    assert info[0]["mask_rbox"].tolist() == [[7, 2], [7, 5], [3, 5], [3, 2]]
    assert info[2]["mask_bbox"] is None and info[2]["mask_rbox"] is None
    lines = open(tmp_path / "rbox" / "t.txt").read().splitlines()
    assert len(lines) == 2                                     # the empty instance has no line
    assert lines[0] == "7.0 2.0 7.0 5.0 3.0 5.0 3.0 2.0 ship 1"
    f = lines[1].split(" ")
    assert len(f) == 10 and f[8:] == ["plane", "0"] and f[:8] == ["%.1f" % v for v in r.mask_rbox[1].reshape(8)]
    # without the new arguments: the keys the pickle always had, and no rbox/ directory
    generate.write_outputs(str(tmp_path / "off"), "t", seg, masks, r.boxes, r.labels, r.areas, pal, names)
    info = pickle.load(open(tmp_path / "off" / "ins" / "t.pkl", "rb"))
    assert sorted(info[0]) == ["bbox", "category", "label", "mask", "size"] and not (tmp_path / "off" / "rbox").exists()


def test_cli_flags():
    from samrs_amd import generate, instances
    base = ["--images", "a", "--boxes", "b", "--out", "c"]
    a = generate.build_parser().parse_args(base)
    assert a.mask_boxes is False and a.dota_txt is False
    a = generate.build_parser().parse_args(base + ["--mask-boxes"])
    assert a.mask_boxes is True and a.dota_txt is False
    a = generate.build_parser().parse_args(base + ["--dota-txt"])
    assert a.mask_boxes is True and a.dota_txt is True         # --dota-txt implies --mask-boxes
    ibase = ["--images", "a", "--annotations", "b", "--out", "c", "--prompt", "box"]
    assert instances.build_parser().parse_args(ibase).mask_boxes is False
    assert instances.build_parser().parse_args(ibase + ["--mask-boxes"]).mask_boxes is True


def test_instances_json_gains_bbox_only_with_the_flag(tmp_path):
    import json
    from samrs_amd import instances
    hb = np.array([[3, 2, 7, 5], [0, 0, 0, 0]], np.int32)
    assert instances.coco_bboxes(hb, [20, 0]) == [[3, 2, 5, 4], [0, 0, 0, 0]]
    on, off = tmp_path / "on", tmp_path / "off"
    kw = dict(pred_area=[20, 0], inter=[10, 0], gt_area=[12, 3], gt_rles=["a", "b"])
    instances.write_fragment(str(on), "s", instances.make_fragment(8, 9, [0.5, 0.25], ["x", "y"], bboxes=[[3, 2, 5, 4], [0, 0, 0, 0]],
                                                                   gt_bboxes=[[1, 1, 4, 3], [2, 2, 1, 3]], **kw))
    instances.write_fragment(str(off), "s", instances.make_fragment(8, 9, [0.5, 0.25], ["x", "y"], **kw))
    instances.merge_fragments(str(on), ["s"], "rhbox", True)
    instances.merge_fragments(str(off), ["s"], "rhbox", True)
    pred = json.load(open(on / "sam_ins_rhbox.json"))
    assert [p["bbox"] for p in pred] == [[3, 2, 5, 4], [0, 0, 0, 0]]
    gt = json.load(open(on / "gt_ins_rhbox.json"))
    assert [a["bbox"] for a in gt["annotations"]] == [[1, 1, 4, 3], [2, 2, 1, 3]]
    assert all("bbox" not in p for p in json.load(open(off / "sam_ins_rhbox.json")))
    assert all("bbox" not in a for a in json.load(open(off / "gt_ins_rhbox.json"))["annotations"])
    for p in pred:
        del p["bbox"]
    assert pred == json.load(open(off / "sam_ins_rhbox.json"))
