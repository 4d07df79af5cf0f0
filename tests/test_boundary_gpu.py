"""GPU: the boundary-band kernels (samrs_mask_boundary_bits) bit for bit against tests/boundary_ref.py, Boundary AP's matching
(samrs_coco_match_min) table for table against the reference's, their argument checks, ``InstancePipeline(boundary=True)``,
``coco_ap.evaluate_files(boundary=True)`` and the two command lines.  Every quantity is an integer count, or a float64 computed from identical integers: all
comparisons are exact."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

from samrs_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import boundary_ref as bref  # noqa: E402
import coco_ap_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _sam(**kw):
    import samrs_amd
    return samrs_amd.sam_model_registry["vit_tiny"](**kw).to("cuda")


@pytest.fixture(scope="module")
def eng():
    sam = _sam(max_images=1, max_prompts=4)
    yield sam.engine


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _disc(h, w, cy, cx, r):
    y, x = np.mgrid[:h, :w]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r * r


def _rect(h, w, y0, x0, hh, ww):
    m = np.zeros((h, w), bool)
    m[max(y0, 0):y0 + hh, max(x0, 0):x0 + ww] = True
    return m


def _masks(h, w, d):
    """Blobs wide enough to keep an interior after d erosions where the image allows it, touching every edge and corner; a mask
    with 1-px holes; all ones; all zero."""
    s = min(h, w)
    holes = np.ones((h, w), bool)
    holes[::max(2 * d + 3, 5), ::max(2 * d + 4, 7)] = False
    holes[0, :] = False
    out = [_disc(h, w, h / 2, w / 2, 0.45 * s), _disc(h, w, h / 3, 2 * w / 3, max(s / 5, d + 2.5)),
           _rect(h, w, 0, 0, 2 * h // 3, 2 * w // 3), _rect(h, w, h // 3, w // 4, h, w), _rect(h, w, 0, w // 2, h, w),
           _rect(h, w, h // 2, 0, h, w // 2 + 1), _rect(h, w, h // 4, 0, h // 2, w), holes, np.ones((h, w), bool), np.zeros((h, w), bool)]
    return np.stack(out)


def _check_bands(eng, masks, h, w, d, want=None):
    planes = eng.pack_mask_bits(torch.from_numpy(masks.view(np.uint8)).cuda())
    keep = planes.clone()
    got = eng.mask_boundary_bits(planes, h, w, d)
    torch.cuda.synchronize()
    assert torch.equal(planes, keep)                                                  # the input is read only
    want = bref.bands(masks, d) if want is None else want
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(masks), (h * w + 63) // 64)
    assert np.array_equal(_u64(got), ref.pack_bits_fast(want))
    if (h * w) % 64:
        assert not np.any(_u64(got)[:, -1] >> np.uint64((h * w) % 64))                # tail bits zero
    return want


SHAPES = [(45, 70, 1), (45, 70, 3), (9, 5, 4), (64, 64, 2), (33, 130, 5), (7, 64, 1), (128, 192, 29)]


@pytest.mark.parametrize("h,w,d", SHAPES, ids=lambda v: str(v))
def test_band_equals_the_reference(eng, h, w, d):
    masks = _masks(h, w, d)
    want = _check_bands(eng, masks, h, w, d)
    if w >= 2 * d + 1 and h >= 2 * d + 1:
        assert (want != masks).any()                                                  # some interior was taken out: not the trivial branch
        frame = np.ones((h, w), bool)
        frame[d:h - d, d:w - d] = False
        assert np.array_equal(want[-2], frame)                                        # all ones: a frame of width d
    else:
        assert np.array_equal(want, masks)                                            # no square fits: the band is the mask
    assert not want[-1].any()


def test_band_of_dense_noise_is_the_noise(eng):
    """The one noise case: a 93 %-dense mask has no (2 d + 1)^2 square set at d = 5, so the band is the mask."""
    rng = np.random.default_rng(5)
    m = (rng.random((2, 33, 130)) < 0.93)
    want = _check_bands(eng, m, 33, 130, 5)
    assert np.array_equal(want, m)


def test_band_at_tile_size(eng):
    h = w = 1024
    m = np.stack([_disc(h, w, 500, 520, 400), _rect(h, w, 0, 0, 700, 1024) | _rect(h, w, 600, 900, 424, 124), _rect(h, w, 90, 100, 57, 61)])
    m[1, 300:301, 400:401] = False                                                    # a 1-px hole
    want = _check_bands(eng, m, h, w, 29)
    assert want[2].sum() == 57 * 61 and want[0].sum() < m[0].sum() // 4              # 57 x 61 < 59 x 59 in one direction: no interior


def test_band_past_64_and_empty_stack(eng):
    h, w, d = 150, 290, 65                                                            # d > 64: the five-word window
    m = np.stack([_rect(h, w, 0, 0, 140, 200), _disc(h, w, 75, 150, 74), np.ones((h, w), bool)])
    _check_bands(eng, m, h, w, d)
    none = torch.zeros(0, (45 * 70 + 63) // 64, dtype=torch.int64, device="cuda")
    assert tuple(eng.mask_boundary_bits(none, 45, 70, 2).shape) == (0, 50)
    planes = torch.zeros(1, 50, dtype=torch.int64, device="cuda")
    out = torch.full((1, 50), 7, dtype=torch.int64, device="cuda")
    assert eng.lib.samrs_mask_boundary_bits(eng.handle, planes.data_ptr(), 0, 45, 70, 2, out.data_ptr(), None) == 0      # n == 0: a no-op
    torch.cuda.synchronize()
    assert (out == 7).all()


def test_band_of_label_planes_equals_band_of_mask_planes(eng):
    h, w, d = 45, 70, 3
    cols = np.array([[10, 20, 30], [200, 100, 0], [10, 20, 30], [1, 2, 3]], dtype=np.uint8)      # a duplicate and an absent colour
    label = np.full((h, w, 3), 128, dtype=np.uint8)
    label[_disc(h, w, 20, 30, 17)] = cols[0]
    label[_rect(h, w, 25, 40, 20, 30)] = cols[1]
    gt = (label[None] == cols[:, None, None, :]).all(-1)
    a = eng.mask_boundary_bits(eng.pack_label_bits(torch.from_numpy(label).cuda(), torch.from_numpy(cols).cuda()), h, w, d)
    b = eng.mask_boundary_bits(eng.pack_mask_bits(torch.from_numpy(gt.view(np.uint8)).cuda()), h, w, d)
    assert torch.equal(a, b) and np.array_equal(_u64(a), ref.pack_bits_fast(bref.bands(gt, d)))
    out = torch.empty_like(a)
    assert eng.mask_boundary_bits(b, h, w, d, out=out) is out and torch.equal(out, a)


# ---- matching ---------------------------------------------------------------------------------------------------------------------
def _match_case():
    """6 detections x 5 ground truths on 96 x 128, d = 3: score ties, a ground truth in the "small" range, and a pair whose mask IoU
    passes 0.75 while its boundary IoU does not."""
    h, w = 96, 128
    gts = np.stack([_disc(h, w, 30, 30, 24), _rect(h, w, 50, 60, 40, 60), _rect(h, w, 2, 70, 20, 30), _disc(h, w, 80, 20, 9),
                    _rect(h, w, 5, 110, 30, 14)])
    preds = np.stack([_disc(h, w, 30, 33, 24), _rect(h, w, 51, 61, 40, 60), _rect(h, w, 2, 70, 20, 30), _disc(h, w, 80, 21, 9),
                      _rect(h, w, 48, 58, 44, 64), _rect(h, w, 60, 0, 10, 10)])
    scores = np.array([0.9, 0.8, 0.8, 0.7, 0.8, 0.6], dtype=np.float32)
    return h, w, 3, preds, scores, gts


def _tables(t):
    order, match, ign, n_valid, n_kept = (v.cpu().numpy() for v in t)
    return {"order": order, "match": match, "dt_ignore": ign, "n_valid": n_valid, "n_kept": int(n_kept[0])}


def test_min_matching_equals_the_reference(eng):
    h, w, d, preds, scores, gts = _match_case()
    assert 0 < gts[3].sum() < 32 ** 2 < gts[0].sum()
    pa = eng.pack_mask_bits(torch.from_numpy(preds.view(np.uint8)).cuda())
    ga = eng.pack_mask_bits(torch.from_numpy(gts.view(np.uint8)).cuda())
    counts = eng.mask_pair_counts(pa, ga)
    band = eng.mask_pair_counts(eng.mask_boundary_bits(pa, h, w, d), eng.mask_boundary_bits(ga, h, w, d))
    host = ref.pair_counts(preds, gts)
    host_b = ref.pair_counts(bref.bands(preds, d), bref.bands(gts, d))
    for got, want in zip(tuple(counts) + tuple(band), host + host_b):
        assert np.array_equal(got.cpu().numpy(), want)
    iou_m, iou_b = bref.iou_matrix(*host), bref.iou_matrix(*host_b)
    assert iou_m[0, 0] >= 0.75 > iou_b[0, 0]                                          # the pair the two metrics disagree on at 0.75
    want = bref.match_counts_min(*host, *host_b, scores)
    got = _tables(eng.coco_match(*counts, torch.from_numpy(scores).cuda(), boundary=band))
    plain_want = ref.match_counts(*host, scores)
    assert not np.array_equal(want["match"], plain_want["match"])                     # the min changes this image's matching
    k = want["n_kept"]
    assert got["n_kept"] == k == 6 and np.array_equal(got["order"][:k], want["order"]) and (got["order"][k:] == -1).all()
    for key in ("match", "dt_ignore", "n_valid"):
        assert np.array_equal(got[key], want[key]), key
    # host scores take the same path
    got_h = _tables(eng.coco_match(*counts, scores, boundary=band))
    for key in ("order", "match", "dt_ignore", "n_valid"):
        assert np.array_equal(got_h[key], got[key]), key
    # boundary=None is today's call, byte for byte, and it is the mask reference's matching
    a = eng.coco_match(*counts, torch.from_numpy(scores).cuda())
    b = eng.coco_match(*counts, torch.from_numpy(scores).cuda(), boundary=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    plain = _tables(b)
    for key in ("match", "dt_ignore", "n_valid"):
        assert np.array_equal(plain[key], plain_want[key]), key
    # a band triple equal to the mask triple changes nothing: min(x, x) = x
    same = _tables(eng.coco_match(*counts, torch.from_numpy(scores).cuda(), boundary=counts))
    for key in ("match", "dt_ignore", "n_valid"):
        assert np.array_equal(same[key], plain_want[key]), key
    # empty sides
    z = lambda *s: torch.zeros(*s, dtype=torch.int64, device="cuda")
    t = _tables(eng.coco_match(z(0, 5), z(0), counts[2], np.zeros(0, np.float32), boundary=(z(0, 5), z(0), band[2])))
    assert t["n_kept"] == 0 and (t["match"] == -1).all() and t["n_valid"].tolist() == plain_want["n_valid"].tolist()


def test_bad_arguments_are_refused(eng):
    import ctypes as C
    from samrs_amd import engine
    lib, hd, bad = eng.lib, eng.handle, engine.ERR_BAD_ARG
    words = (45 * 70 + 63) // 64
    planes = torch.zeros(2, words, dtype=torch.int64, device="cuda")
    out = torch.full((2, words), 7, dtype=torch.int64, device="cuda")
    call = lambda p=planes.data_ptr(), n=2, h=45, w=70, d=2, o=out.data_ptr(), e=hd: lib.samrs_mask_boundary_bits(e, p, n, h, w, d, o, None)
    assert call(e=None) == bad and call(p=None) == bad and call(o=None) == bad and call(n=-1) == bad
    assert call(d=0) == bad and call(d=129) == bad and call(d=-3) == bad
    assert call(h=0) == bad and call(w=0) == bad and call(h=1 << 15, w=1 << 15) == bad
    assert call(o=planes.data_ptr()) == bad and call(o=planes.data_ptr() + 8 * words) == bad       # the output overlaps the input
    assert b"samrs_mask_boundary_bits" in lib.samrs_last_error(hd)
    torch.cuda.synchronize()
    assert (out == 7).all() and (planes == 0).all()                                   # nothing was launched: nothing written
    assert call(d=128) == engine.OK and call(d=1) == engine.OK
    torch.cuda.synchronize()
    assert (out == 0).all()
    with pytest.raises(AssertionError, match="1..128"):
        eng.mask_boundary_bits(planes, 45, 70, 0)
    with pytest.raises(ValueError, match="planes"):
        eng.mask_boundary_bits(planes, 45, 90, 2)                                     # 64 words per plane, not 50

    thr = (C.c_double * 10)(*ref.THRESHOLDS.tolist())
    rng_ = (C.c_double * 8)(*np.asarray(ref.RANGES, dtype=np.float64).reshape(-1).tolist())
    order = torch.full((100,), 7, dtype=torch.int32, device="cuda")
    match = torch.full((4, 10, 100), 7, dtype=torch.int32, device="cuda")
    ign = torch.full((4, 10, 100), 7, dtype=torch.uint8, device="cuda")
    nv = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    nk = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    inter = torch.ones(2, 2, dtype=torch.int64, device="cuda")
    area = torch.full((2,), 2, dtype=torch.int64, device="cuda")
    sc = torch.tensor([0.5, 0.25], device="cuda")

    def cm(inter_b=inter.data_ptr(), area_db=area.data_ptr(), area_gb=area.data_ptr(), inter_p=inter.data_ptr(), nd=2, ng=2, T=10,
           order_p=order.data_ptr(), max_det=100):
        return lib.samrs_coco_match_min(hd, inter_p, area.data_ptr(), area.data_ptr(), inter_b, area_db, area_gb, sc.data_ptr(), 0, nd, ng,
                                        thr, T, rng_, 4, max_det, order_p, match.data_ptr(), ign.data_ptr(), nv.data_ptr(), nk.data_ptr(), None)
    assert cm(inter_b=None) == bad and cm(area_db=None) == bad and cm(area_gb=None) == bad and cm(inter_p=None) == bad
    assert cm(nd=-1) == bad and cm(T=17) == bad and cm(order_p=None) == bad and cm(max_det=0) == bad
    assert b"samrs_coco_match_min" in lib.samrs_last_error(hd)
    torch.cuda.synchronize()
    for t in (order, match, ign, nv, nk):
        assert (t == 7).all()
    assert cm() == engine.OK
    torch.cuda.synchronize()
    assert int(nk[0]) == 2 and order[:3].tolist() == [0, 1, -1]
    with pytest.raises(ValueError, match="boundary"):
        eng.coco_match(inter, area, area, sc, boundary=(inter, area))
    with pytest.raises(ValueError, match="area_gb"):
        eng.coco_match(inter, area, area, sc, boundary=(inter, area, area[:1]))


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _items():
    import test_instances_gpu as tig
    from samrs_amd import driver
    items = []
    for i, (h, w) in enumerate([(320, 448), (261, 389)]):                              # d = 11 and 9; 261 x 389 is no multiple of 64
        img = synth.make_image(70 + i, h, w)
        polys, labels = synth.make_rboxes(70 + i, 6, h, w)
        polys = (polys * 0.6 + np.array([w, h], np.float32) * 0.2).astype(np.float32)      # towards the middle: boxes with an interior
        cols = tig._colors(6, 70 + i)
        label = tig._paint_labels(h, w, polys, cols)
        items.append(driver.WorkItem(f"b{i}", img, polys, labels, (label, cols)))
    return items


def _collect(pipe, items):
    from samrs_amd import driver
    got = {}

    def sink(results, release):
        for r in results:
            n = len(r.labels)
            rec = {f.name: getattr(r, f.name) for f in dataclasses.fields(r) if not f.name.endswith("_data")}
            rec = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in rec.items()}
            rec["rles"] = [r.rle(j) for j in range(n)]
            rec["gt_rles"] = [r.gt_rle(j) for j in range(n)]
            for name in ("ap_tables", "boundary_tables"):
                t = getattr(r, name)
                rec[name] = None if t is None else {k: (np.array(v) if not isinstance(v, int) else v) for k, v in t.items()}
            got[r.key] = rec
        release()
    assert pipe.run(driver.batched(items, 2), sink) == len(items)
    return got


def _same(a, b):
    if isinstance(a, dict) and isinstance(b, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return a is not None and b is not None and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return a == b


def test_instance_pipeline_boundary_tables_equal_the_reference():
    import test_instances_gpu as tig
    from samrs_amd import coco_ap, driver
    sam = _sam(max_images=4, max_prompts=4)
    items = _items()
    kw = dict(prompt="box", multimask=False, batch=2, box_batch=4, max_boxes=8, rle=True, rle_buffer_mb=16, keep_masks=True, gt=True, ap=True)
    with pytest.raises(ValueError, match="ap=True"):
        driver.InstancePipeline(sam, 1, prompt="box", multimask=False, batch=2, gt=True, boundary=True)
    off = _collect(driver.InstancePipeline(sam, 1, boundary=False, **kw), items)
    on = _collect(driver.InstancePipeline(sam, 1, boundary=True, **kw), items)       # 6 boxes in chunks of 4: planes span chunks
    new = {"boundary_order", "boundary_match", "boundary_dt_ignore", "boundary_n_valid", "boundary_n_kept", "band_inter", "band_area_d",
           "band_area_g", "boundary_tables"}
    for it in items:
        a, c = off[it.key], on[it.key]
        assert set(a) == set(c)
        for k in a:
            if k in new:
                assert a[k] is None and c[k] is not None, (it.key, k)
            else:
                assert _same(a[k], c[k]), (it.key, k)                                 # boundary=True changes no other output, ap_tables included
        label, cols = it.gt
        gt = tig._gt_numpy(label, cols)
        h, w = label.shape[:2]
        d = coco_ap.boundary_dilation(h, w)
        assert d == bref.dilation(h, w) and h >= 2 * d + 1
        want = bref.match_masks_min(c["masks"], c["quality"], gt, d)
        t = c["boundary_tables"]
        k = want["n_kept"]
        assert t["n_kept"] == k == 6 and np.array_equal(t["order"][:k], want["order"]) and (t["order"][k:] == -1).all()
        assert np.array_equal(t["match"], want["match"]) and np.array_equal(t["dt_ignore"], want["dt_ignore"])
        assert np.array_equal(t["n_valid"], want["n_valid"]) and np.array_equal(t["scores"], c["quality"].astype(np.float64))
        bp, bg = bref.bands(c["masks"], d), bref.bands(gt, d)
        assert bp.sum() > 0 and (bg != gt).any()                                      # the painted boxes have an interior: real bands
        assert t["band_inter"].dtype == np.int64 and t["band_inter"].tolist() == [int((p & g).sum()) for p, g in zip(bp, bg)]
        assert t["band_area_d"].tolist() == bp.sum((1, 2)).tolist() and t["band_area_g"].tolist() == bg.sum((1, 2)).tolist()


def test_evaluate_files_boundary_equals_the_reference(eng, tmp_path):
    from samrs_amd import coco_ap, rle
    images = []
    for k, (h, w) in enumerate([(96, 128), (70, 45)]):
        rng = np.random.default_rng(40 + k)
        gts = np.stack([_disc(h, w, h * 0.3, w * 0.3, 0.22 * min(h, w)), _rect(h, w, h // 2, w // 3, h // 3, w // 2), _rect(h, w, 2, w - 14, 9, 12)])
        preds = np.stack([np.roll(gts[0], (1, 2), (0, 1)), _rect(h, w, h // 2 + 1, w // 3 - 2, h // 3, w // 2), np.roll(gts[2], 1, 0),
                          _disc(h, w, h * 0.8, w * 0.15, 5)])
        images.append((preds, rng.choice([0.9, 0.7, 0.5], 4).astype(np.float32), gts))
    dt, gt = [], {"images": [], "annotations": [], "categories": [{"id": 0, "name": "ship"}]}
    for n, (p, s, g) in enumerate(images):
        gt["images"].append({"id": n, "height": int(p.shape[1]), "width": int(p.shape[2])})
        dt += [{"image_id": n, "category_id": 0, "segmentation": rle.encode(m), "score": float(sc)} for m, sc in zip(p, s)]
        gt["annotations"] += [{"id": c, "image_id": n, "category_id": 0, "segmentation": rle.encode(m), "area": int(m.sum()), "iscrowd": 0}
                              for c, m in enumerate(g)]
    dt_path, gt_path = str(tmp_path / "dt.json"), str(tmp_path / "gt.json")
    json.dump(dt, open(dt_path, "w"))
    json.dump(gt, open(gt_path, "w"))
    want, want_tables = bref.evaluate(images)
    got, tables = coco_ap.evaluate_files(eng, dt_path, gt_path, boundary=True)
    for a, b in zip(tables, want_tables):
        for key in ("order", "match", "dt_ignore", "n_valid"):
            assert np.array_equal(a[key], np.asarray(b[key])[..., :len(a["order"])] if key in ("match", "dt_ignore") else b[key]), key
    assert set(got) == set(ref.NAMES)
    for k in ref.NAMES:
        assert got[k] == want[k], (k, got[k], want[k])                                # float64 equality: identical integers in
    mask_numbers, _ = coco_ap.evaluate_files(eng, dt_path, gt_path)
    assert mask_numbers == coco_ap.accumulate(ref.evaluate(images)[1]) and mask_numbers["AP"] > got["AP"]
    rec = coco_ap.ap_record(got, tables, boundary=True)
    assert rec["iou"] == "min(mask, boundary)" and rec["n_dt"] == 8 and rec["n_gt"] == 6


def test_instances_cli_boundary_and_the_coco_ap_tool(tmp_path, capsys):
    import test_instances_gpu as tig
    from samrs_amd import coco_ap, instances, rle
    img_dir, ann_dir, lab_dir, sizes = tig._write_dataset(str(tmp_path))
    tig._paint_dataset_labels(img_dir, ann_dir, lab_dir, sizes)
    base, out = str(tmp_path / "base"), str(tmp_path / "out")
    instances.main(tig._cli_args(img_dir, ann_dir, lab_dir, base, "box", ["--ap"]))
    before = capsys.readouterr().out.splitlines()
    instances.main(tig._cli_args(img_dir, ann_dir, lab_dir, out, "box", ["--ap", "--boundary"]))          # 7 objects, --box-batch 4
    lines = capsys.readouterr().out.splitlines()
    for name in ("miou.json", "ap.json", "sam_ins_rhbox.json", "gt_ins_rhbox.json"):                       # unchanged by the flag
        assert open(os.path.join(out, name), "rb").read() == open(os.path.join(base, name), "rb").read(), name
    assert not os.path.exists(os.path.join(base, "boundary_ap.json"))
    rec = json.load(open(os.path.join(out, "boundary_ap.json")))
    assert rec["matching"] == "by index" and rec["iou"] == "min(mask, boundary)" and rec["dilation_ratio"] == 0.02
    assert rec["n_images"] == 3 and rec["n_gt"] == 21 and rec["n_dt"] == 21 and sorted(rec["boundary_miou"]) == ["area", "average"]
    at0 = [i for i, ln in enumerate(before) if ln.startswith("Average mIOU:")][0]
    at = [i for i, ln in enumerate(lines) if ln.startswith("Average mIOU:")][0]
    assert lines[at:at + 13] == before[at0:at0 + 13] and len(before) == at0 + 13                           # the existing output comes first
    assert len(lines) == at + 27
    assert lines[at + 13].startswith("Boundary AP") and lines[at + 14:at + 26] == coco_ap.summary_lines(rec)
    assert lines[at + 26].startswith("Boundary mIOU")
    # the fragments: the record, the diagonal band counts, and --resume
    frags = {s: json.load(open(os.path.join(out, "parts", s + ".json"))) for s in ("s0", "s1", "s2")}
    frag = frags["s0"]
    assert sorted(frag["boundary_ap"]) == ["dt_ignore", "match", "n_valid", "order"] and len(frag["boundary_ap"]["order"]) == 7
    assert all(len(frag[k]) == 7 for k in ("band_inter", "band_area_d", "band_area_g"))
    dt = json.load(open(os.path.join(out, "sam_ins_rhbox.json")))
    gt = json.load(open(os.path.join(out, "gt_ins_rhbox.json")))
    n0 = [im["id"] for im in gt["images"] if im["file_name"] == "s0.png"][0]                               # 517 x 803: d = 19
    preds = np.stack([rle.decode(d["segmentation"]) for d in dt if d["image_id"] == n0])
    gts = np.stack([rle.decode(g["segmentation"]) for g in gt["annotations"] if g["image_id"] == n0])
    d0 = bref.dilation(517, 803)
    bp, bg = bref.bands(preds, d0), bref.bands(gts, d0)
    assert frag["band_inter"] == [int((p & g).sum()) for p, g in zip(bp, bg)]
    assert frag["band_area_d"] == bp.sum((1, 2)).tolist() and frag["band_area_g"] == bg.sum((1, 2)).tolist()
    want0 = bref.match_masks_min(preds, np.array(frag["scores"], np.float32), gts, d0)
    assert frag["boundary_ap"]["match"] == want0["match"][:, :, :7].tolist() and frag["boundary_ap"]["order"] == want0["order"].tolist()
    # Boundary mIoU over the objects miou.json covers, from the fragments' integers
    allf = [frags[s] for s in sorted(frags)]
    cat = lambda k: [v for fr in allf for v in fr[k]]
    cov = [j for j, (i, p, g) in enumerate(zip(cat("inter"), cat("pred_area"), cat("gt_area"))) if p + g - i > 0]
    assert len(cov) == json.load(open(os.path.join(out, "miou.json")))["n_instances"]
    bi, bd, bgs = (np.array(cat(k), dtype=np.int64)[cov] for k in ("band_inter", "band_area_d", "band_area_g"))
    un = bd + bgs - bi
    per = [float(i) / float(u) if u > 0 else 0.0 for i, u in zip(bi, un)]
    assert rec["boundary_miou"]["average"] == float(np.mean(per)) and rec["boundary_miou"]["area"] == float(bi.sum() / un.sum())
    del frag["boundary_ap"]
    json.dump(frag, open(os.path.join(out, "parts", "s0.json"), "w"))
    os.remove(os.path.join(out, "boundary_ap.json"))
    instances.main(tig._cli_args(img_dir, ann_dir, lab_dir, out, "box", ["--ap", "--boundary", "--resume"]))
    assert "2 of 3 images already complete" in capsys.readouterr().out
    assert json.load(open(os.path.join(out, "boundary_ap.json"))) == rec
    # the stand-alone tool on the two files gives the same twelve numbers and counts
    out2 = str(tmp_path / "b2.json")
    argv = ["--dt", os.path.join(out, "sam_ins_rhbox.json"), "--gt", os.path.join(out, "gt_ins_rhbox.json")]
    rec2 = coco_ap.main(argv + ["--boundary", "--out", out2])
    printed = capsys.readouterr().out.splitlines()
    assert rec2 == {k: v for k, v in rec.items() if k != "boundary_miou"} and json.load(open(out2)) == rec2
    assert printed[-13].startswith("Boundary AP") and printed[-12:] == coco_ap.summary_lines(rec)
    assert coco_ap.main(argv) == json.load(open(os.path.join(out, "ap.json")))                            # without the flag: unchanged
    assert len(capsys.readouterr().out.splitlines()) == 12
