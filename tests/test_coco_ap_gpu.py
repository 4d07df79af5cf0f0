"""GPU: COCO mask AP on the device (ap_kernels.hip) -- the bit-plane packs, the pairwise counts and the greedy matching alone, each
against numpy / tests/coco_ap_ref.py for exact equality, then the chain through InstancePipeline(ap=True), ``samrs_amd.instances
--ap`` and ``python -m samrs_amd.coco_ap``.  Integer work and correctly rounded divisions on both sides: every table is compared
exactly; the twelve numbers to 1e-12 (float64 means of at most 1010 values in [0, 1]: they can differ by rounding order only).

Two notes on the constructed matching cases.  ``np.linspace(.5, .95, 10)[2]`` is exactly 0.6 with the numpy in use (older releases
gave 0.6000000000000001), so the k / 20 case runs twice: with COCO's thresholds as numpy gives them, and with the third one set to
0.6000000000000001, where 3 / 5 must not match.  Areas of exactly 9216 do not fit a 64 x 64 mask: that case is 128 x 128."""
import dataclasses
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from samrs_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coco_ap_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _sam(**kw):
    import samrs_amd
    return samrs_amd.sam_model_registry["vit_tiny"](**kw).to("cuda")


@pytest.fixture(scope="module")
def eng():
    sam = _sam(max_images=1, max_prompts=4)
    yield sam.engine


def _on_device(arr, aligned):
    """The array's bytes on the device, contiguous; unaligned: a slice that starts at an odd byte of its allocation."""
    a = np.ascontiguousarray(arr)
    if aligned:
        t = torch.from_numpy(a).cuda()
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.empty(a.size + 1, dtype=torch.uint8, device="cuda")
    t = buf[1:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 2 == 1 and t.is_contiguous()
    return t


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


# ---- pack -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [False, True], ids=["odd-byte", "aligned"])
@pytest.mark.parametrize("h,w,n", [(1, 1, 3), (7, 9, 3), (37, 53, 3), (64, 64, 3), (1024, 1024, 2)])
def test_pack_mask_bits_equals_numpy(eng, h, w, n, aligned):
    rng = np.random.default_rng(h * 131 + w)
    masks = rng.choice(np.array([0, 1, 255], dtype=np.uint8), size=(n, h, w))
    masks[0, -1, -1] = 255                                                        # the last pixel: the tail word's top used bit
    words = (h * w + 63) // 64
    out = torch.full((n + 2, words), -1, dtype=torch.int64, device="cuda")      # all ones: the tail bits must be cleared
    got = eng.pack_mask_bits(_on_device(masks, aligned), out[1:n + 1])
    torch.cuda.synchronize()
    want = ref.pack_bits_fast(masks)
    assert np.array_equal(_u64(got), want)
    if h * w % 64:
        assert not np.any(_u64(got)[:, -1] >> np.uint64(h * w % 64))
    assert (out[0] == -1).all() and (out[n + 1] == -1).all()
    fresh = eng.pack_mask_bits(_on_device(masks != 0, aligned).view(torch.bool))   # bool masks, a new output
    assert fresh.dtype == torch.int64 and np.array_equal(_u64(fresh), want)


@pytest.mark.parametrize("h,w,n", [(1, 1, 2), (7, 9, 4), (37, 53, 300), (64, 64, 5), (1024, 1024, 2)])
def test_pack_label_bits_equals_numpy(eng, h, w, n):
    rng = np.random.default_rng(h + 7 * w)
    palette = rng.integers(0, 256, size=(6, 3), dtype=np.uint8)
    label = palette[rng.integers(0, 6, size=(h, w))]
    colors = palette[rng.integers(0, 6, size=n)].astype(np.uint8)
    colors[0] = [7, 7, 7]                                                         # absent from the image
    assert not (label == colors[0]).all(-1).any()
    colors[-1] = colors[1] if n > 2 else colors[-1]                               # duplicated
    out = torch.full((n, (h * w + 63) // 64), -1, dtype=torch.int64, device="cuda")
    got = eng.pack_label_bits(_on_device(label, False), _on_device(colors, False), out)
    torch.cuda.synchronize()
    gt = ref.label_masks(label, colors)
    assert np.array_equal(_u64(got), ref.pack_bits_fast(gt))
    assert not _u64(got)[0].any() and (n <= 2 or np.array_equal(_u64(got)[-1], _u64(got)[1]))


# ---- pair counts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na,nb,h,w", [(0, 3, 37, 53), (1, 1, 37, 53), (3, 0, 37, 53), (5, 2, 37, 53), (70, 33, 37, 53), (130, 130, 37, 53),
                                        (8, 8, 1024, 1024)])
def test_mask_pair_counts_equal_the_integer_product(eng, na, nb, h, w):
    rng = np.random.default_rng(na * 1000 + nb)
    a = (rng.random((na, h, w)) < rng.random((na, 1, 1))).astype(np.uint8)
    b = (rng.random((nb, h, w)) < rng.random((nb, 1, 1))).astype(np.uint8)
    words = (h * w + 63) // 64
    empty = lambda: torch.zeros(0, words, dtype=torch.int64, device="cuda")
    pa = eng.pack_mask_bits(torch.from_numpy(a).cuda()) if na else empty()
    pb = eng.pack_mask_bits(torch.from_numpy(b).cuda()) if nb else empty()
    inter, aa, ab = eng.mask_pair_counts(pa, pb)
    torch.cuda.synchronize()
    fa, fb = a.reshape(na, h * w).astype(np.int64), b.reshape(nb, h * w).astype(np.int64)
    assert inter.shape == (na, nb) and np.array_equal(inter.cpu().numpy(), fa @ fb.T)
    assert np.array_equal(aa.cpu().numpy(), fa.sum(1)) and np.array_equal(ab.cpu().numpy(), fb.sum(1))
    if na and nb:                                                                 # the outputs are overwritten, not accumulated
        eng.mask_pair_counts(pa, pb, inter, aa, ab)
        assert np.array_equal(inter.cpu().numpy(), fa @ fb.T) and np.array_equal(aa.cpu().numpy(), fa.sum(1))
        same, _, _ = eng.mask_pair_counts(pa, pa)                                 # a plane set against itself
        assert np.array_equal(same.cpu().numpy(), fa @ fa.T)


@pytest.mark.parametrize("n,h,w", [(5, 37, 53), (8, 1024, 1024)])
def test_pair_counts_diagonal_agrees_with_gt_match(eng, n, h, w):
    rng = np.random.default_rng(n)
    palette = rng.integers(0, 256, size=(4, 3), dtype=np.uint8)
    label = torch.from_numpy(palette[rng.integers(0, 4, size=(h, w))]).cuda()
    colors = torch.from_numpy(palette[rng.integers(0, 4, size=n)].astype(np.uint8)).cuda()
    masks = torch.from_numpy((rng.random((n, h, w)) < 0.4).astype(np.uint8) * 255).cuda()
    inter, gta, _ = eng.gt_match(masks, label, colors)
    pi, pa, pg = eng.mask_pair_counts(eng.pack_mask_bits(masks), eng.pack_label_bits(label, colors))
    assert torch.equal(pi.diagonal(), inter) and torch.equal(pg, gta)
    assert torch.equal(pa, (masks != 0).flatten(1).sum(1))


# ---- matching ---------------------------------------------------------------------------------------------------------------------
def _device_tables(eng, preds, scores, gts, thresholds=None, hw=(64, 64)):
    preds = np.asarray(preds, dtype=np.uint8).reshape(-1, *hw)
    gts = np.asarray(gts, dtype=np.uint8).reshape(-1, *hw)
    words = (hw[0] * hw[1] + 63) // 64
    empty = lambda: torch.zeros(0, words, dtype=torch.int64, device="cuda")
    pa = eng.pack_mask_bits(torch.from_numpy(preds).cuda()) if len(preds) else empty()
    pb = eng.pack_mask_bits(torch.from_numpy(gts).cuda()) if len(gts) else empty()
    inter, ad, ag = eng.mask_pair_counts(pa, pb)
    sc = torch.tensor(np.asarray(scores, dtype=np.float32).reshape(-1), device="cuda")
    order, match, ign, n_valid, n_kept = eng.coco_match(inter, ad, ag, sc, thresholds=thresholds)
    return {"order": order.cpu().numpy(), "match": match.cpu().numpy(), "dt_ignore": ign.cpu().numpy(), "n_valid": n_valid.cpu().numpy(),
            "n_kept": int(n_kept.cpu()[0])}


def _check(eng, preds, scores, gts, thresholds=None, hw=(64, 64)):
    """Every table of the device equals the reference's; returns the reference's tables."""
    kw = {} if thresholds is None else {"thresholds": thresholds}
    preds = np.asarray(preds, dtype=np.uint8).reshape(-1, *hw)
    gts = np.asarray(gts, dtype=np.uint8).reshape(-1, *hw)
    want = ref.match_masks(preds, scores, gts, **kw)
    got = _device_tables(eng, preds, scores, gts, thresholds, hw)
    k = want["n_kept"]
    assert got["n_kept"] == k
    assert np.array_equal(got["order"][:k], want["order"]) and (got["order"][k:] == -1).all()
    assert np.array_equal(got["n_valid"], want["n_valid"])
    assert got["match"].shape == want["match"].shape and got["match"].dtype == np.int32 and got["dt_ignore"].dtype == np.uint8
    assert np.array_equal(got["match"], want["match"])
    assert np.array_equal(got["dt_ignore"], want["dt_ignore"])
    return want


def _rows(hw=(64, 64)):
    return np.zeros(hw, np.uint8)


def test_match_ious_exactly_on_the_thresholds(eng):
    """Pair r: a ground truth of 20 pixels and a prediction of k = 10 + r of them: IoU exactly k / 20, no other overlap."""
    preds, gts = [], []
    for r, k in enumerate(range(10, 20)):
        g, p = _rows(), _rows()
        g[3 * r, :20] = 1
        p[3 * r, :k] = 1
        gts.append(g)
        preds.append(p)
    scores = np.linspace(0.9, 0.1, 10)
    want = _check(eng, preds, scores, gts)
    thr = ref.THRESHOLDS
    for r, k in enumerate(range(10, 20)):                                         # the reference itself, against plain float64
        assert want["match"][0, :, r].tolist() == [r if np.float64(k) / np.float64(20) >= thr[t] else -1 for t in range(10)]
    older = ref.THRESHOLDS.copy()
    older[2] = 0.6000000000000001
    want = _check(eng, preds, scores, gts, thresholds=older)
    assert want["match"][0, :, 2].tolist() == [2, 2] + [-1] * 8                   # 12 / 20 = 3 / 5 is below 0.6000000000000001
    assert want["match"][0, 2, 3] == 3                                            # 13 / 20 is not


def test_match_equal_ious_and_equal_scores(eng):
    p = _rows()
    p[5, :20] = 1
    g0, g1 = _rows(), _rows()
    g0[5, :10] = 1
    g1[5, 10:20] = 1                                                              # both 10 / 20
    want = _check(eng, [p], [0.5], [g0, g1])
    assert want["match"][0, 0, 0] == 1                                            # the later ground truth on a tie
    q = _rows()
    q[5, :10] = 1                                                                 # equal scores: index order; the second takes what is left
    want = _check(eng, [q, p, q], [0.5, 0.5, 0.5], [g0, g1])
    assert want["order"].tolist() == [0, 1, 2] and want["match"][0, 0, :3].tolist() == [0, 1, -1]
    _check(eng, [q, p, q], [0.25, 0.5, 0.5], [g0, g1])


def test_match_max_det_and_many_ground_truths(eng):
    rng = np.random.default_rng(5)
    gts, preds = [], []
    for j in range(70):                                                           # more ground truths than a wave has lanes
        g = _rows()
        y, x = 4 * (j // 8), 8 * (j % 8)
        g[y:y + 3, x:x + 6] = 1
        gts.append(g)
    for d in range(130):
        p = gts[d % 70].copy()
        p[rng.integers(0, 64), rng.integers(0, 64)] ^= 1
        if d % 3 == 0:
            p = np.roll(p, 2, axis=1)
        preds.append(p)
    scores = np.round(rng.random(130), 2)                                         # ties among them
    want = _check(eng, preds, scores, gts)
    assert want["n_kept"] == 100 and (want["match"][0, 0] >= 0).sum() > 40


def test_match_inclusive_area_range_ends(eng):
    hw = (128, 128)
    g0, g1, g2 = _rows(hw), _rows(hw), _rows(hw)
    g0[:32, :32] = 1                                                              # 1024: small AND medium
    g1[32:128, 32:128] = 1                                                        # 9216: medium AND large
    g2[40:50, :10] = 1
    preds = [g0.copy(), g1.copy(), g2.copy()]
    want = _check(eng, preds, [0.9, 0.8, 0.7], [g0, g1, g2], hw=hw)
    assert want["n_valid"].tolist() == [3, 2, 2, 1]
    assert want["dt_ignore"][:, 0, :3].tolist() == [[0, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1]]


def test_match_a_detection_that_can_only_match_an_ignored_ground_truth(eng):
    hw = (128, 128)
    small, big = _rows(hw), _rows(hw)
    small[:10, :10] = 1                                                           # 100 px: ignored in the medium and large ranges
    big[20:60, 20:60] = 1                                                         # 1600 px: medium
    d0 = small.copy()
    d1 = _rows(hw)
    d1[20:60, 20:45] = 1                                                          # IoU 1000 / 1600 with big: below 0.65 and up
    want = _check(eng, [d0, d1], [0.9, 0.8], [small, big], hw=hw)
    assert want["match"][2, 0, :2].tolist() == [0, 1] and want["dt_ignore"][2, 0, :2].tolist() == [1, 0]
    assert want["match"][2, 5, :2].tolist() == [0, -1]


def test_match_union_zero_and_empty_sides(eng):
    e = _rows()
    g = _rows()
    g[:4, :4] = 1
    want = _check(eng, [e], [0.5], [e])                                           # empty against empty: IoU 0, no match
    assert (want["match"][:, :, 0] == -1).all()
    _check(eng, [e, g], [0.5, 0.4], [e, g])
    want = _check(eng, [], [], [g, g])                                            # nd = 0
    assert want["n_kept"] == 0 and want["n_valid"].tolist() == [2, 2, 0, 0]
    want = _check(eng, [g, e], [0.1, 0.2], [])                                    # ng = 0
    assert want["n_kept"] == 2 and want["n_valid"].tolist() == [0, 0, 0, 0] and want["order"].tolist() == [1, 0]
    _check(eng, [], [], [])


def _blobs(rng, n, hw=(64, 64)):
    out = []
    y, x = np.mgrid[:hw[0], :hw[1]]
    for _ in range(n):
        cy, cx, ry, rx = rng.integers(0, hw[0]), rng.integers(0, hw[1]), rng.integers(1, 24), rng.integers(1, 24)
        out.append((((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2 <= 1).astype(np.uint8))
    return out


def test_match_random_blob_images(eng):
    rng = np.random.default_rng(2024)
    images = []
    for _ in range(40):
        gts = _blobs(rng, int(rng.integers(0, 7)))
        preds = []
        for g in gts:
            if rng.random() < 0.8:
                preds.append(np.roll(g, int(rng.integers(-3, 4)), axis=int(rng.integers(0, 2))) if rng.random() < 0.7 else g.copy())
        preds += _blobs(rng, int(rng.integers(0, 4)))
        scores = np.round(rng.random(len(preds)), 1).astype(np.float32)
        want = _check(eng, preds, scores, gts)
        images.append((np.asarray(preds, np.uint8).reshape(-1, 64, 64), scores, np.asarray(gts, np.uint8).reshape(-1, 64, 64)))
    # the whole evaluation through the public function: the twelve numbers against the reference
    from samrs_amd import coco_ap
    got, tables = coco_ap.evaluate_masks(eng, images)
    want, _ = ref.evaluate(images)
    for k in ref.NAMES:
        assert got[k] == pytest.approx(want[k], abs=1e-12), (k, got[k], want[k])
    assert len(tables) == 40 and want["AP"] > 0


def test_bad_arguments_are_refused(eng):
    from samrs_amd import engine
    import ctypes as C
    lib, h = eng.lib, eng.handle
    m = torch.zeros(2, 8, 8, dtype=torch.uint8, device="cuda")
    planes = torch.zeros(2, 1, dtype=torch.int64, device="cuda")
    lab = torch.zeros(8, 8, 3, dtype=torch.uint8, device="cuda")
    col = torch.zeros(2, 3, dtype=torch.uint8, device="cuda")
    bad = engine.ERR_BAD_ARG
    assert lib.samrs_mask_pack_bits(h, None, 2, 8, 8, planes.data_ptr(), None) == bad
    assert lib.samrs_mask_pack_bits(h, m.data_ptr(), 2, 8, 8, None, None) == bad
    assert lib.samrs_mask_pack_bits(h, m.data_ptr(), -1, 8, 8, planes.data_ptr(), None) == bad
    assert lib.samrs_mask_pack_bits(h, m.data_ptr(), 2, 0, 8, planes.data_ptr(), None) == bad
    assert lib.samrs_mask_pack_bits(h, m.data_ptr(), 2, 1 << 15, 1 << 15, planes.data_ptr(), None) == bad
    assert b"samrs_mask_pack_bits" in lib.samrs_last_error(h)
    assert lib.samrs_mask_pack_bits(h, m.data_ptr(), 0, 8, 8, planes.data_ptr(), None) == engine.OK
    assert lib.samrs_label_pack_bits(h, None, col.data_ptr(), 2, 8, 8, planes.data_ptr(), None) == bad
    assert lib.samrs_label_pack_bits(h, lab.data_ptr(), None, 2, 8, 8, planes.data_ptr(), None) == bad
    assert lib.samrs_label_pack_bits(h, lab.data_ptr(), col.data_ptr(), -2, 8, 8, planes.data_ptr(), None) == bad
    assert lib.samrs_label_pack_bits(h, lab.data_ptr(), col.data_ptr(), 0, 8, 8, planes.data_ptr(), None) == engine.OK
    inter = torch.zeros(2, 2, dtype=torch.int64, device="cuda")
    area = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert lib.samrs_mask_pair_counts(h, None, 2, planes.data_ptr(), 2, 1, inter.data_ptr(), None, None, None) == bad
    assert lib.samrs_mask_pair_counts(h, planes.data_ptr(), 2, planes.data_ptr(), 2, 1, None, None, None, None) == bad
    assert lib.samrs_mask_pair_counts(h, planes.data_ptr(), -1, planes.data_ptr(), 2, 1, inter.data_ptr(), None, None, None) == bad
    assert lib.samrs_mask_pair_counts(h, planes.data_ptr(), 2, planes.data_ptr(), 2, 0, inter.data_ptr(), None, None, None) == bad
    assert lib.samrs_mask_pair_counts(h, None, 0, None, 0, 1, None, None, None, None) == engine.OK
    thr = (C.c_double * 10)(*ref.THRESHOLDS.tolist())
    rng_ = (C.c_double * 8)(*np.asarray(ref.RANGES, dtype=np.float64).reshape(-1).tolist())
    order = torch.full((100,), 7, dtype=torch.int32, device="cuda")
    match = torch.full((4, 10, 100), 7, dtype=torch.int32, device="cuda")
    ign = torch.full((4, 10, 100), 7, dtype=torch.uint8, device="cuda")
    nv = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    nk = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    sc = torch.tensor([0.5, 0.25], device="cuda")

    def call(inter_p=inter.data_ptr(), scores=sc.data_ptr(), on_host=0, nd=2, ng=2, thr_p=thr, T=10, order_p=order.data_ptr(), max_det=100):
        return lib.samrs_coco_match(h, inter_p, area.data_ptr(), area.data_ptr(), scores, on_host, nd, ng, thr_p, T, rng_, 4, max_det,
                                    order_p, match.data_ptr(), ign.data_ptr(), nv.data_ptr(), nk.data_ptr(), None)
    assert call(inter_p=None) == bad and call(scores=None) == bad and call(order_p=None) == bad and call(thr_p=None) == bad
    assert call(nd=-1) == bad and call(ng=-1) == bad and call(T=0) == bad and call(T=17) == bad and call(max_det=0) == bad
    host = (C.c_float * 2)(0.5, float("nan"))
    assert call(scores=C.cast(host, C.c_void_p), on_host=1) == bad and b"NaN" in lib.samrs_last_error(h)
    torch.cuda.synchronize()
    for t in (order, match, ign, nv, nk):                                         # nothing was launched: nothing written
        assert (t == 7).all()
    with pytest.raises(AssertionError, match="NaN"):
        eng.coco_match(inter, area, area, np.array([0.5, np.nan], np.float32))
    host_ok = (C.c_float * 2)(0.25, 0.5)                                          # host scores are uploaded by the call
    assert call(scores=C.cast(host_ok, C.c_void_p), on_host=1) == engine.OK
    torch.cuda.synchronize()
    assert order[:3].tolist() == [1, 0, -1] and int(nk[0]) == 2
    sc[1] = float("nan")                                                          # device scores cannot be read by the host: flagged
    assert call() == engine.OK
    torch.cuda.synchronize()
    assert int(nk[0]) == -1 and (match == -1).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _items(prompt="box"):
    import test_instances_gpu as tig
    from samrs_amd import driver
    items = []
    for i, (h, w) in enumerate([(1024, 1024), (600, 800), (517, 803)]):
        img = synth.make_image(60 + i, h, w)
        polys, labels = synth.make_rboxes(60 + i, 9, h, w)
        cols = tig._colors(9, 60 + i)
        label = tig._paint_labels(h, w, polys, cols)
        items.append(driver.WorkItem(f"t{i}", img, polys, labels, (label, cols)))
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
            rec["ap_tables"] = None if r.ap_tables is None else {k: (np.array(v) if not isinstance(v, int) else v) for k, v in r.ap_tables.items()}
            got[r.key] = rec
        release()
    assert pipe.run(driver.batched(items, 2), sink) == len(items)
    return got


def _same(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return a is not None and b is not None and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
    return a == b


def test_instance_pipeline_ap_tables_equal_the_reference():
    import test_instances_gpu as tig
    from samrs_amd import driver
    sam = _sam(max_images=4, max_prompts=4)
    items = _items()
    kw = dict(prompt="box", multimask=False, batch=2, box_batch=4, max_boxes=16, rle=True, rle_buffer_mb=16, keep_masks=True, gt=True)
    with pytest.raises(ValueError, match="gt=True"):
        driver.InstancePipeline(sam, 1, prompt="box", multimask=False, batch=2, ap=True)
    plain = _collect(driver.InstancePipeline(sam, 1, **kw), items)
    off = _collect(driver.InstancePipeline(sam, 1, ap=False, **kw), items)
    on = _collect(driver.InstancePipeline(sam, 1, ap=True, **kw), items)                # 9 boxes in chunks of 4: planes span chunks
    ap_fields = {"ap_order", "ap_match", "ap_dt_ignore", "ap_n_valid", "ap_n_kept", "ap_tables"}
    for it in items:
        a, b, c = plain[it.key], off[it.key], on[it.key]
        assert set(a) == set(b) == set(c)
        for k in a:
            assert _same(a[k], b[k]), (it.key, k)                                 # ap=False: every field as without the option
            if k in ap_fields:
                assert a[k] is None and c[k] is not None, (it.key, k)
            else:
                assert _same(a[k], c[k]), (it.key, k)                             # ap=True changes no other output
        label, cols = it.gt
        want = ref.match_masks(c["masks"], c["quality"], tig._gt_numpy(label, cols))
        t = c["ap_tables"]
        k = want["n_kept"]
        assert t["n_kept"] == k == 9 and np.array_equal(t["order"][:k], want["order"]) and (t["order"][k:] == -1).all()
        assert np.array_equal(t["match"], want["match"]) and np.array_equal(t["dt_ignore"], want["dt_ignore"])
        assert np.array_equal(t["n_valid"], want["n_valid"]) and np.array_equal(t["scores"], c["quality"].astype(np.float64))


def test_instances_cli_ap_and_the_coco_ap_tool(tmp_path, capsys):
    import test_instances_gpu as tig
    from samrs_amd import coco_ap, instances, rle
    img_dir, ann_dir, lab_dir, sizes = tig._write_dataset(str(tmp_path))
    tig._paint_dataset_labels(img_dir, ann_dir, lab_dir, sizes)
    out = str(tmp_path / "out")
    instances.main(tig._cli_args(img_dir, ann_dir, lab_dir, out, "box", ["--ap"]))            # 7 objects, --box-batch 4
    printed = capsys.readouterr().out
    rec = json.load(open(os.path.join(out, "ap.json")))
    assert rec["matching"] == "by index" and rec["n_images"] == 3 and rec["n_gt"] == 21 and rec["n_dt"] == 21
    dt = json.load(open(os.path.join(out, "sam_ins_rhbox.json")))
    gt = json.load(open(os.path.join(out, "gt_ins_rhbox.json")))
    images = []
    for im in gt["images"]:
        ds = [d for d in dt if d["image_id"] == im["id"]]
        gs = [g for g in gt["annotations"] if g["image_id"] == im["id"]]
        images.append((np.stack([rle.decode(d["segmentation"]) for d in ds]), np.array([d["score"] for d in ds], np.float32),
                       np.stack([rle.decode(g["segmentation"]) for g in gs])))
    want, _ = ref.evaluate(images)
    for k in ref.NAMES:
        assert rec[k] == pytest.approx(want[k], abs=1e-12), (k, rec[k], want[k])
    lines = printed.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("Average mIOU:")]
    assert at and lines[at[0] + 1:at[0] + 13] == coco_ap.summary_lines(rec)
    frag = json.load(open(os.path.join(out, "parts", "s0.json")))
    assert sorted(frag["ap"]) == ["dt_ignore", "match", "n_valid", "order"] and len(frag["ap"]["order"]) == 7
    # --resume under --ap: a fragment written without the record counts as not done
    del frag["ap"]
    json.dump(frag, open(os.path.join(out, "parts", "s0.json"), "w"))
    os.remove(os.path.join(out, "ap.json"))
    instances.main(tig._cli_args(img_dir, ann_dir, lab_dir, out, "box", ["--ap", "--resume"]))
    assert json.load(open(os.path.join(out, "ap.json"))) == rec
    # the stand-alone tool on the two files
    capsys.readouterr()
    out2 = str(tmp_path / "ap2.json")
    rec2 = coco_ap.main(["--dt", os.path.join(out, "sam_ins_rhbox.json"), "--gt", os.path.join(out, "gt_ins_rhbox.json"), "--out", out2])
    assert rec2 == rec and json.load(open(out2)) == rec
    assert capsys.readouterr().out.splitlines()[-12:] == coco_ap.summary_lines(rec)
