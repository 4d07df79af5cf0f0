"""Host side of the instances CLI (samrs_amd.instances): the HRSC XML reader, the mIoU from per-instance tallies, the COCO JSON
merge of the per-image fragments and its --resume bookkeeping.  Where the reference tree is present its own ``load_hrsc`` and
``instance_to_json`` are imported (with a cv2 stub and a pycocotools shim backed by samrs_amd.rle) and must agree bit for bit /
character for character."""
import importlib
import json
import math
import os
import sys
import types

import numpy as np
import pytest

from samrs_amd import driver, instances, rle


def _obj(cx, cy, w, h, ang, color="10,20,30", box=(0, 0, 1, 1)):
    return {"box_xmin": box[0], "box_ymin": box[1], "box_xmax": box[2], "box_ymax": box[3], "mbox_cx": cx, "mbox_cy": cy,
            "mbox_w": w, "mbox_h": h, "mbox_ang": ang, "seg_color": color}


def _write_xml(path, objs):
    rows = ["<HRSC_Object><Object_ID>1</Object_ID>" + "".join(f"<{k}>{v}</{k}>" for k, v in o.items()) + "</HRSC_Object>"
            for o in objs]
    with open(path, "w") as f:
        f.write("<?xml version='1.0'?><HRSC_Image><Img_ID>1</Img_ID><HRSC_Objects>" + "".join(rows) + "</HRSC_Objects></HRSC_Image>")


def _cases(d):
    """name -> objects of hand-written annotation files."""
    rng = np.random.default_rng(7)
    many = [_obj(f"{rng.uniform(0, 1000):.4f}", f"{rng.uniform(0, 600):.4f}", f"{rng.uniform(5, 300):.4f}", f"{rng.uniform(5, 80):.4f}",
                 f"{rng.uniform(-math.pi / 2, math.pi / 2):.6f}", "{},{},{}".format(*rng.integers(0, 256, 3)),
                 tuple(int(v) for v in rng.integers(0, 900, 4))) for _ in range(40)]
    return {
        "zero": [_obj("100", "50", "40", "20", "0", "1,2,3", (80, 40, 120, 60))],
        "right": [_obj("100", "50", "40", "20", "1.5707963", " 255, 0,7")],
        "many": many,
        "nocolor": [_obj("100", "50", "40", "20", "0"), _obj("10", "20", "4", "2", "0.3", "12,34")],
        "empty": [],
    }


def test_xml_reader_known_answers(tmp_path):
    for name, objs in _cases(tmp_path).items():
        _write_xml(str(tmp_path / f"{name}.xml"), objs)
    a = instances.read_hrsc_xml(str(tmp_path / "zero.xml"))
    assert not a.skip
    assert a.rboxes.dtype == np.float32 and a.rboxes.shape == (1, 4, 2)
    assert np.array_equal(a.rboxes[0], np.array([[80, 40], [120, 40], [120, 60], [80, 60]], np.float32))
    assert np.array_equal(a.points, np.array([[100, 50]], np.float32)) and np.array_equal(a.colors, np.array([[1, 2, 3]], np.uint8))
    assert np.array_equal(a.hboxes, np.array([[80, 40, 120, 60]], np.float32))
    # angle pi/2: the le90 corners start at (110, 30) (top right); the best begin point moves the start to the top-left corner
    r = instances.read_hrsc_xml(str(tmp_path / "right.xml"))
    assert np.allclose(r.rboxes[0], [[90, 30], [110, 30], [110, 70], [90, 70]], atol=1e-4)
    raw0 = np.array([100 + 10, 50 - 20])
    assert not np.allclose(r.rboxes[0, 0], raw0, atol=1e-3) and np.allclose(r.rboxes[0, 1], raw0, atol=1e-3)
    assert np.array_equal(r.colors, np.array([[255, 0, 7]], np.uint8))
    # a colour without three fields or an image without objects skips the whole image
    assert instances.read_hrsc_xml(str(tmp_path / "nocolor.xml")).skip
    assert instances.read_hrsc_xml(str(tmp_path / "empty.xml")).skip
    assert not instances.read_hrsc_xml(str(tmp_path / "many.xml")).skip


def test_list_images_skips_like_the_reference(tmp_path):
    img, ann = tmp_path / "img", tmp_path / "ann"
    img.mkdir()
    ann.mkdir()
    for name, objs in _cases(tmp_path).items():
        _write_xml(str(ann / f"{name}.xml"), objs)
        (img / f"{name}.bmp").write_bytes(b"")
    (img / "orphan.bmp").write_bytes(b"")                  # no annotation file: ignored
    (img / "notes.txt").write_bytes(b"")
    stems, files, anns = instances.list_images(str(img), str(ann))
    assert stems == ["many", "right", "zero"] and files["zero"] == "zero.bmp" and set(anns) == set(stems)


# ------------------------------------------------------------------------------------------------
# the reference's own functions
# ------------------------------------------------------------------------------------------------
@pytest.fixture()
def reference_modules():
    from oracle import ref_import
    if not ref_import.reference_available():
        pytest.skip("the reference tree is not present")
    names = ("cv2", "pycocotools", "pycocotools.mask", "loaddata", "mapping", "utils", "utils.transform", "instance_to_json")
    saved = {n: sys.modules.pop(n) for n in names if n in sys.modules}
    cv2 = types.ModuleType("cv2")                          # utils/transform.py imports it; load_hrsc does not use it
    pc, pcm = types.ModuleType("pycocotools"), types.ModuleType("pycocotools.mask")

    def encode(m):
        d = rle.encode(np.asarray(m))
        return {"size": d["size"], "counts": d["counts"].encode("ascii")}

    pcm.encode, pc.mask = encode, pcm
    sys.modules.update({"cv2": cv2, "pycocotools": pc, "pycocotools.mask": pcm})
    sys.path.insert(0, ref_import.REF_ROOT)
    dont = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        yield importlib.import_module("loaddata"), importlib.import_module("instance_to_json")
    finally:
        sys.dont_write_bytecode = dont
        sys.path.remove(ref_import.REF_ROOT)
        for n in names:
            sys.modules.pop(n, None)
        sys.modules.update(saved)


def test_xml_reader_equals_reference_load_hrsc(tmp_path, reference_modules):
    loaddata, _ = reference_modules
    for name, objs in _cases(tmp_path).items():
        _write_xml(str(tmp_path / f"{name}.xml"), objs)
        hb, rb, col, pt, lab, err = loaddata.load_hrsc(name, str(tmp_path))
        a = instances.read_hrsc_xml(str(tmp_path / f"{name}.xml"))
        assert a.skip == (err == 1), name
        assert len(rb) == len(a.rboxes) and lab == [0] * len(rb)
        for j in range(len(rb)):
            for mine, ref in ((a.hboxes[j], hb[j]), (a.rboxes[j], rb[j]), (a.colors[j], col[j]), (a.points[j], pt[j])):
                assert mine.dtype == ref.dtype and mine.shape == ref.shape, name
                assert mine.tobytes() == ref.tobytes(), f"{name} object {j}: {mine} != {ref}"


def _fragments_case(seed=3):
    rng = np.random.default_rng(seed)
    stems = ["b07", "a01", "c11"]
    sizes = {"a01": (5, 7), "b07": (6, 4), "c11": (9, 9)}
    pm, gm, q = {}, {}, {}
    for s in stems:
        h, w = sizes[s]
        n = int(rng.integers(1, 5))
        pm[s] = rng.random((n, h, w)) < 0.4
        gm[s] = rng.random((n, h, w)) < 0.3
        gm[s][0] = False
        pm[s][0] = False                                   # an instance with an empty union
        q[s] = rng.random(n).astype(np.float32)
    return stems, sizes, pm, gm, q


def _write_case(out, stems, sizes, pm, gm, q, with_gt=True):
    for s in stems:
        h, w = sizes[s]
        p, g = pm[s], gm[s]
        rles = [rle.encode(m)["counts"] for m in p]
        if with_gt:
            frag = instances.make_fragment(h, w, q[s], rles, p.reshape(len(p), -1).sum(1), (p & g).reshape(len(p), -1).sum(1),
                                           g.reshape(len(g), -1).sum(1), [rle.encode(m)["counts"] for m in g])
        else:
            frag = instances.make_fragment(h, w, q[s], rles)
        instances.write_fragment(out, s, frag)


def test_json_writers_equal_reference_instance_to_json(tmp_path, reference_modules):
    _, itj = reference_modules
    stems, sizes, pm, gm, q = _fragments_case()
    out = str(tmp_path)
    _write_case(out, stems, sizes, pm, gm, q)
    order = sorted(stems)
    instances.merge_fragments(out, order, "rbox", with_gt=True)
    want_pred = itj.binary_to_coco_pre_hrsc([pm[s] for s in order], order, all_probs=[q[s] for s in order])
    want_gt = itj.binary_to_coco_gt_hrsc([gm[s].astype(np.uint8) for s in order], order)
    assert open(os.path.join(out, "sam_ins_rbox.json")).read() == json.dumps(want_pred)
    assert open(os.path.join(out, "gt_ins_rbox.json")).read() == json.dumps(want_gt)


def test_miou_from_tallies_equals_mean_iou():
    stems, sizes, pm, gm, q = _fragments_case(5)
    inter, pa, ga = [], [], []
    for s in stems:
        p, g = pm[s], gm[s]
        inter += list((p & g).reshape(len(p), -1).sum(1))
        pa += list(p.reshape(len(p), -1).sum(1))
        ga += list(g.reshape(len(g), -1).sum(1))
    avg, area, k = instances.miou_from_tallies(inter, pa, ga)
    want = driver.mean_iou([pm[s] for s in stems], [gm[s] for s in stems])
    assert (avg, area) == want                               # exactly: the same floats in the same order
    assert k == sum(len(pm[s]) for s in stems) - len(stems)   # one empty-union instance per image is left out
    assert all(math.isnan(v) for v in instances.miou_from_tallies([0], [0], [0])[:2])


def test_fragment_merge_ids_order_and_resume(tmp_path, capsys):
    stems, sizes, pm, gm, q = _fragments_case(11)
    out = str(tmp_path)
    order = sorted(stems)
    assert instances.pending_stems(out, order) == order
    _write_case(out, stems[:2], sizes, pm, gm, q)
    assert instances.pending_stems(out, order) == ["c11"]
    with pytest.raises(RuntimeError, match="c11"):
        instances.merge_fragments(out, order, "hbox", with_gt=True)
    _write_case(out, stems[2:], sizes, pm, gm, q)
    assert instances.pending_stems(out, order) == []
    rec = instances.merge_fragments(out, order, "hbox", with_gt=True)
    pred = json.load(open(os.path.join(out, "sam_ins_hbox.json")))
    gt = json.load(open(os.path.join(out, "gt_ins_hbox.json")))
    assert [im["file_name"] for im in gt["images"]] == [f"{s}.png" for s in order] and [im["id"] for im in gt["images"]] == [0, 1, 2]
    assert [(im["height"], im["width"]) for im in gt["images"]] == [sizes[s] for s in order]
    want_ids = [(n, c) for n, s in enumerate(order) for c in range(len(gm[s]))]
    assert [(a["image_id"], a["id"]) for a in gt["annotations"]] == want_ids          # ids restart per image
    assert [p["image_id"] for p in pred] == [n for n, c in want_ids]
    assert [p["score"] for p in pred] == [float(v) for s in order for v in q[s]]
    for a, (n, c) in zip(gt["annotations"], want_ids):
        g = gm[order[n]][c]
        assert a["area"] == int(g.sum()) and np.array_equal(rle.decode(a["segmentation"]), g)
        assert a["category_id"] == 0 and a["iscrowd"] == 0 and a["attributes"] == {}
    assert rec == json.load(open(os.path.join(out, "miou.json")))
    avg, area = driver.mean_iou([pm[s] for s in order], [gm[s] for s in order])
    assert rec["average"] == avg and rec["area"] == area
    assert f"Average mIOU:  {avg} Area mIOU:  {area}" in capsys.readouterr().out
    # without ground truth: the predictions only
    out2 = str(tmp_path / "nogt")
    _write_case(out2, stems, sizes, pm, gm, q, with_gt=False)
    assert instances.merge_fragments(out2, order, "hbox", with_gt=False) is None
    assert open(os.path.join(out2, "sam_ins_hbox.json")).read() == open(os.path.join(out, "sam_ins_hbox.json")).read()
    assert sorted(os.listdir(out2)) == ["parts", "sam_ins_hbox.json"]
