"""CPU: the host halves of the RLE decode path -- rle.pack_strings (the layout samrs_rle_decode reads), the relabel CLI's parser and
generate.write_outputs(base_entries=...), which lets an existing pickle's keys survive a rewrite."""
import os
import pickle

import numpy as np
import pytest

from samrs_amd import generate, rle


def _masks():
    rng = np.random.default_rng(41)
    a = rng.random((13, 29)) < 0.4
    b = np.zeros((13, 29), bool)
    c = np.ones((13, 29), bool)
    return [a, b, c]


def test_pack_strings_layout_and_counts_forms():
    masks = _masks()
    strs = [rle.encode(m)["counts"] for m in masks]
    forms = [{"size": [13, 29], "counts": strs[0]},                                        # str
             {"size": [13, 29], "counts": strs[1].encode("ascii")},                        # bytes, as pycocotools returns
             {"size": [13, 29], "counts": rle.mask_to_counts(masks[2])},                   # uncompressed
             {"size": [13, 29], "counts": ""}]
    buf, table = rle.pack_strings(forms)
    assert buf.dtype == np.uint8 and table.dtype == np.int64 and table.shape == (4, 3)
    assert (table[:, 0] % 16 == 0).all() and (table[:, 2] == 0).all()
    assert table[:, 1].tolist() == [len(strs[0]), len(strs[1]), len(strs[2]), 0]
    for j in range(3):
        assert table[j + 1, 0] >= table[j, 0] + table[j, 1]                                # packed in order, no overlap
    assert len(buf) % 16 == 0 and len(buf) >= table[3, 0] + table[3, 1]
    for j, m in enumerate(masks):
        s = buf[table[j, 0]:table[j, 0] + table[j, 1]].tobytes().decode("ascii")
        assert s == strs[j]
        assert rle.string_to_counts(s) == rle.mask_to_counts(m)                            # the round trip
        assert np.array_equal(rle.decode({"size": [13, 29], "counts": s}), m)
    buf0, table0 = rle.pack_strings([])
    assert buf0.size == 0 and table0.shape == (0, 3)


def test_relabel_parser_accepts_its_options(tmp_path):
    from samrs_amd import relabel
    ins = tmp_path / "a" / "ins"
    ins.mkdir(parents=True)
    ap = relabel.build_parser()
    ns = ap.parse_args(["--ins", str(tmp_path / "a"), "--out", str(tmp_path / "b"), "--n-classes", "5", "--min-region-area", "16",
                        "--region-mode", "holes", "--overlap", "smallest", "--dota-txt", "--polygons", "--polygon-max-edges", "999",
                        "--png-device", "--resume", "--box-batch", "7"])
    assert ns.min_region_area == 16 and ns.region_mode == "holes" and ns.overlap == "smallest" and ns.dota_txt and ns.mask_boxes
    assert ns.polygons and ns.polygon_max_edges == 999 and ns.png_device and ns.resume and ns.box_batch == 7 and ns.n_classes == 5
    ns = ap.parse_args(["--ins", str(tmp_path / "a"), "--out", str(tmp_path / "b")])
    assert ns.overlap == "order" and ns.min_region_area == 0 and not ns.mask_boxes and not ns.png_device and not ns.resume
    # a generate output directory is read through its ins/; a directory of pickles as it is
    assert relabel.ins_dir_of(str(tmp_path / "a")) == str(ins)
    (ins / "x.pkl").write_bytes(pickle.dumps([]))
    assert relabel.ins_dir_of(str(ins)) == str(ins)


@pytest.mark.parametrize("extra,word", [(["--overlap", "logit"], "logits"), (["--quality"], "logits"), (["--min-stability", "0.9"], "logits"),
                                        (["--min-pred-iou", "0.5"], "logits"), (["--min-inside-box", "0.5"], "logits"),
                                        (["--vis"], "image"), (None, "input directory")])
def test_relabel_parser_refuses_what_the_pickles_cannot_give(tmp_path, capsys, extra, word):
    from samrs_amd import relabel
    (tmp_path / "a" / "ins").mkdir(parents=True)
    out = tmp_path / "b"
    if extra is None:                                                       # --out whose ins/ is the input directory
        extra, out = [], tmp_path / "a"
    with pytest.raises(SystemExit) as ex:
        relabel.build_parser().parse_args(["--ins", str(tmp_path / "a"), "--out", str(out)] + extra)
    assert ex.value.code == 2 and word in capsys.readouterr().err


def _write(tmp_path, name, **kw):
    masks = np.stack(_masks())
    labels = np.array([2, 0, 1])
    areas = masks.reshape(3, -1).sum(1)
    seg = np.full((13, 29), 255, np.uint8)
    for m, l in zip(masks, labels):
        seg[m] = l
    boxes = np.array([[0, 0, 5, 5], [1, 1, 6, 6], [2, 2, 7, 7]], np.float32)
    out = tmp_path / name
    generate.write_outputs(str(out), "T0", seg, masks, boxes, labels, areas, generate.default_palette(3), ["a", "b", "c"], **kw)
    return out, masks, areas


def test_write_outputs_base_entries_keep_foreign_keys(tmp_path):
    base = [{"bbox": [9, 9, 9, 9], "category": "ship", "label": 7, "size": -1, "mask": {"size": [1, 1], "counts": "1"},
             "rbox": np.arange(8, dtype=np.float32).reshape(4, 2), "rhbox": [1, 2, 3, 4], "note": {"k": j}} for j in range(3)]
    keep = pickle.loads(pickle.dumps(base))
    rbs = [np.full((4, 2), j, np.float32) for j in range(3)]
    out, masks, areas = _write(tmp_path, "o", base_entries=base, mask_bboxes=[[0, 0, 1, 1]] * 3, mask_rboxes=rbs, removed=[4, 5, 6])
    got = pickle.load(open(out / "ins" / "T0.pkl", "rb"))
    assert len(got) == 3
    for j, e in enumerate(got):
        assert list(e)[:8] == list(base[j])                                 # every input key, in its order
        assert e["bbox"] == [9, 9, 9, 9] and e["category"] == "ship" and e["label"] == 7 and e["rhbox"] == [1, 2, 3, 4]
        assert np.array_equal(e["rbox"], keep[j]["rbox"]) and e["note"] == {"k": j}
        assert e["size"] == int(areas[j]) and type(e["size"]) is int        # replaced by those of the masks as they go out
        assert e["mask"] == rle.encode(masks[j])
        assert e["mask_bbox"] == [0, 0, 1, 1] and np.array_equal(e["mask_rbox"], rbs[j]) and e["removed"] == 4 + j
    for j, e in enumerate(base):                                            # the caller's entries are copied, not edited
        assert e["size"] == -1 and e["mask"] == {"size": [1, 1], "counts": "1"} and "mask_bbox" not in e


def test_write_outputs_without_base_entries_is_unchanged(tmp_path):
    out, masks, areas = _write(tmp_path, "o")
    got = pickle.load(open(out / "ins" / "T0.pkl", "rb"))
    assert [list(e) for e in got] == [["bbox", "category", "label", "size", "mask"]] * 3
    for j, e in enumerate(got):
        assert e["category"] == ["c", "a", "b"][j] and e["label"] == [2, 0, 1][j] and e["size"] == int(areas[j])
        assert np.array_equal(e["bbox"], np.array([[0, 0, 5, 5], [1, 1, 6, 6], [2, 2, 7, 7]], np.float32)[j])
        assert e["mask"] == rle.encode(masks[j])
    out2, _, _ = _write(tmp_path, "o2", base_entries=None)
    assert open(out / "ins" / "T0.pkl", "rb").read() == open(out2 / "ins" / "T0.pkl", "rb").read()
    for sub in ("gray", "color"):
        assert os.path.exists(out / sub / "T0.png")
