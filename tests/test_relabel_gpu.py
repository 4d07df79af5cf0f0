"""GPU: ``python -m samrs_amd.relabel`` -- every mask-only output re-derived from ins/*.pkl without an encoder pass -- against the
generate run that wrote the pickles (vit_tiny, the three-tile dataset of tests/test_png_device_gpu.py).  Everything downstream of the
masks is integer work on the device: the comparisons are exact."""
import json
import os
import pickle
import shutil

import numpy as np
import pytest

import overlap_ref
import test_png_device_gpu as tp
from samrs_amd import rle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gen(tmp_path_factory):
    """(root, img_dir, boxes, A): generate run once into A"""
    from samrs_amd import generate
    root = tmp_path_factory.mktemp("relabel")
    img_dir, boxes = tp._cli_dataset(root)
    a = root / "A"
    generate.run(tp._cli_args(img_dir, boxes, a))
    return root, img_dir, boxes, a


def _relabel(ins, out, *extra):
    from samrs_amd import relabel
    return relabel.run(relabel.build_parser().parse_args(["--ins", str(ins), "--out", str(out), "--n-classes", "18", "--box-batch", "20"]
                                                         + list(extra)))


def _pkl(d, stem):
    return pickle.load(open(os.path.join(d, "ins", stem + ".pkl"), "rb"))


def _same_value(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same_value(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def _same_entries(da, db, stems):
    for s in stems:
        ea, eb = _pkl(da, s), _pkl(db, s)
        assert len(ea) == len(eb) and len(ea) > 0, s
        for j, (x, y) in enumerate(zip(ea, eb)):
            assert list(x) == list(y), (s, j)                               # the same keys
            for k in x:
                assert _same_value(x[k], y[k]), (s, j, k)                   # RLE strings, sizes, box arrays, ...


def _same_maps(da, db):
    ta, tb = tp._tree(da), tp._tree(db)
    maps = sorted(k for k in ta if k.startswith(("gray", "color")))
    assert len(maps) == 6 and maps == sorted(k for k in tb if k.startswith(("gray", "color")))
    for k in maps:
        assert ta[k] == tb[k], k


def _same_statistics(da, db):
    sa, sb = (json.load(open(os.path.join(d, "statistic", "class_stats.json"))) for d in (da, db))
    for k in ("class_pixel_num", "class_instance_num", "mask_num"):
        assert sa[k] == sb[k], k
    assert sb["source"] == "ins"
    size = lambda d: np.load(os.path.join(d, "statistic", "all_mask_size.npy"))
    assert np.array_equal(size(da), size(db))
    return sa, sb


STEMS = ["P0000", "P0001", "P0002"]


@pytest.mark.parametrize("png_device", [False, True])
def test_relabel_with_defaults_reproduces_the_run(gen, png_device):
    root, _, _, a = gen
    b = root / f"B{int(png_device)}"
    _relabel(a, b, *(["--png-device"] if png_device else []))
    _same_maps(a, b)
    _same_entries(a, b, STEMS)
    _same_statistics(a, b)
    assert sorted(os.listdir(b)) == ["color", "gray", "ins", "statistic"]


def test_relabel_clean_up_and_dota_equal_a_generate_run(gen):
    from samrs_amd import generate
    root, img_dir, boxes, a = gen
    g, r = root / "G_clean", root / "R_clean"
    generate.run(tp._cli_args(img_dir, boxes, g, min_region_area=16, dota_txt=True))
    _relabel(a / "ins", r, "--min-region-area", "16", "--dota-txt")          # a directory of pickles as it is
    _same_maps(g, r)
    _same_entries(g, r, STEMS)                                              # with mask_bbox / mask_rbox
    assert all("mask_rbox" in e for e in _pkl(r, "P0001"))
    sg, sr = _same_statistics(g, r)
    assert sg["region_cleanup"] == sr["region_cleanup"] and sr["region_cleanup"]["changed_pixel_num"] > 0
    tg, tr = tp._tree(g), tp._tree(r)
    txt = sorted(k for k in tg if k.startswith("rbox"))
    assert len(txt) == 3 and txt == sorted(k for k in tr if k.startswith("rbox"))
    for k in txt:
        assert tg[k] == tr[k] and len(tg[k]) > 0, k


def test_relabel_overlap_smallest_matches_the_reference_rule(gen):
    root, _, _, a = gen
    r = root / "R_small"
    from samrs_amd import generate, tile_io
    stats = _relabel(a, r, "--overlap", "smallest")
    total = hit = 0
    for s in STEMS:
        ea, er = _pkl(a, s), _pkl(r, s)
        masks = np.stack([rle.decode(e["mask"]) for e in ea])
        want, _, _, removed = overlap_ref.resolve(masks, None, overlap_ref.primary(masks, "smallest"))
        want = want != 0
        assert len(er) == len(ea)
        for j, e in enumerate(er):
            assert e["mask"] == rle.encode(want[j]), (s, j)
            assert e["size"] == int(want[j].sum()) and e["removed"] == int(removed[j]) and type(e["removed"]) is int
            assert np.array_equal(e["bbox"], ea[j]["bbox"]) and e["label"] == ea[j]["label"]
        seg = overlap_ref.paint(want, [e["label"] for e in ea])
        # the files the default writer makes of that map
        tile_io.write_label_pair(str(root / "want_gray.png"), str(root / "want_color.png"), seg, tile_io.class_lut(generate.default_palette(18)))
        for sub in ("gray", "color"):
            assert open(r / sub / f"{s}.png", "rb").read() == open(root / f"want_{sub}.png", "rb").read(), (s, sub)
        total += int(removed.sum())
        hit += int((removed > 0).sum())
    assert total > 0 and stats["overlap"] == {"rule": "smallest", "removed_pixel_num": total, "removed_instance_num": hit}


def test_relabel_resume_recreates_a_deleted_image(gen):
    root, _, _, a = gen
    r = root / "R_resume"
    _relabel(a, r)
    before = tp._tree(r)
    for sub, ext in (("gray", ".png"), ("color", ".png"), ("ins", ".pkl")):
        os.remove(r / sub / ("P0001" + ext))
    marker = r / "gray" / "P0000.png"
    t0 = os.stat(marker).st_mtime_ns
    _relabel(a, r, "--resume")
    after = tp._tree(r)
    assert sorted(after) == sorted(before)
    for k in before:
        if k.endswith("all_mask_size.npy"):                                 # the finished images' sizes come first: same sizes, other order
            assert sorted(np.load(r / k).tolist()) == sorted(np.load(a / k).tolist())
        else:
            assert after[k] == before[k], k
    assert os.stat(marker).st_mtime_ns == t0                                # a finished image was not written again


def test_relabel_keeps_foreign_keys_and_refuses_foreign_labels(gen):
    from samrs_amd import relabel
    root, _, _, a = gen
    src = root / "foreign"
    src.mkdir()
    # published-style pickles of another size than A's, with a rotated box and a key this project never writes
    rng = np.random.default_rng(5)
    entries = []
    for j in range(5):
        m = np.zeros((70, 99), bool)
        m[5 + 9 * j: 30 + 9 * j, 7 + 11 * j: 50 + 11 * j] = True
        m[12 + 9 * j: 16 + 9 * j, 20 + 11 * j: 25 + 11 * j] = False         # a hole
        m &= rng.random(m.shape) < 0.97
        entries.append({"bbox": [7 + 11 * j, 5 + 9 * j, 43, 25], "category": "ship", "label": j % 3, "size": int(m.sum()),
                        "mask": rle.encode(m), "rbox": np.full((4, 2), j, np.float32), "note": f"n{j}"})
    pickle.dump(entries, open(src / "Q.pkl", "wb"))
    out = root / "R_foreign"
    _relabel(src, out, "--mask-boxes", "--polygons")
    got = _pkl(out, "Q")
    assert len(got) == len(entries)
    for j, (e, x) in enumerate(zip(got, entries)):
        assert np.array_equal(e["rbox"], x["rbox"]) and e["note"] == f"n{j}" and e["mask"] == x["mask"] and e["size"] == x["size"]
        assert "mask_bbox" in e and "polygons" in e and "polygon_holes" in e
    from samrs_amd import polygons
    for e in got:
        assert any(e["polygon_holes"])
        rings = list(zip(e["polygons"], e["polygon_holes"]))
        assert np.array_equal(polygons.rasterize(rings, 70, 99), rle.decode(e["mask"]).astype(np.uint8))
    # a label outside the class list: refused, naming the file
    bad = root / "badlabel"
    bad.mkdir()
    entries[3]["label"] = 18
    pickle.dump(entries, open(bad / "Z7.pkl", "wb"))
    with pytest.raises(ValueError, match=r"Z7\.pkl.*label 18"):
        _relabel(bad, root / "R_bad")
    # an entry without its mask, and mixed sizes
    del entries[3]["mask"]
    entries[3]["label"] = 1
    pickle.dump(entries, open(bad / "Z7.pkl", "wb"))
    with pytest.raises(ValueError, match=r"Z7\.pkl.*entry 3 has no"):
        _relabel(bad, root / "R_bad")
    entries[3]["mask"] = rle.encode(np.ones((4, 4), bool))
    pickle.dump(entries, open(bad / "Z7.pkl", "wb"))
    with pytest.raises(ValueError, match=r"Z7\.pkl.*mixed sizes"):
        _relabel(bad, root / "R_bad")
    with pytest.raises(ValueError, match="input directory"):
        relabel.run(relabel.argparse.Namespace(ins=str(a), out=str(a), overlap="order", quality=False, min_stability=0.0, min_pred_iou=0.0,
                                               min_inside_box=0.0, vis=False))
    shutil.rmtree(bad)
