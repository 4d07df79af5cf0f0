"""GPU: samrs_score_masks / samrs_filter_masks (quality_kernels.hip) alone, then the scores through SamPredictor, TilePipeline and
the generation CLI.

Kernel level (vit_tiny engine, low = 4 * randn(3, 256, 256), seed 3, offsets 1.0 and 0.25, the five shapes of quality_ref.SHAPES):
the counts are integers, so every comparison against the engine's own postprocess output is exact; against the host reference
(F.interpolate twice) the counts may differ by the pixels whose reference logit lies within 1e-5 of the threshold (quality_ref's
band), and the test first asserts that this band is small.  filter_masks runs on (5, 67, 93) masks at an odd base address (byte
stores) and on (3, 70, 272) masks (16-byte stores)."""
import functools
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from samrs_amd import quality, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import quality_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N_CLASSES = 18
SHAPES, OFFSETS = quality_ref.SHAPES, quality_ref.OFFSETS
SHAPE_IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SHAPES]


@functools.lru_cache(maxsize=None)
def _weights():
    """Seeded weights with a checkpoint-like logit spread (synth.MARGIN_LOGIT_SCALE): with the plain synthetic weights every logit
    lies within +-0.5, so no pixel exceeds +1 and every stability is 0 -- nothing for a threshold to separate."""
    return synth.make_state_dict(synth.CONFIGS["vit_tiny"], 0, logit_scale=synth.MARGIN_LOGIT_SCALE)


def _sam(name="vit_tiny", **kw):
    import samrs_amd
    return samrs_amd.sam_model_registry[name](state_dict=_weights(), **kw).to("cuda")


@pytest.fixture(scope="module")
def eng():
    sam = _sam(max_images=1, max_prompts=4)
    yield sam.engine


@functools.lru_cache(maxsize=None)
def _low():
    return quality_ref.make_low(3, 3)


@functools.lru_cache(maxsize=None)
def _ref(k: int):
    """The host reference logits of shape k, computed once and shared."""
    return quality_ref.logits(_low(), *SHAPES[k])


_engine_out = {}


def _engine(eng, k: int):
    """(fp32 logits, uint8 masks) of the engine's own postprocess for shape k, on the host; computed once and shared."""
    if k not in _engine_out:
        (ih, iw), (oh, ow) = SHAPES[k]
        low = _low().cuda()
        L = torch.empty(3, oh, ow, dtype=torch.float32, device="cuda")
        M = torch.empty(3, oh, ow, dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        assert eng.lib.samrs_k_postprocess(low.data_ptr(), 3, ih, iw, oh, ow, 1024, 1, L.data_ptr(), s) == 0
        assert eng.lib.samrs_k_postprocess(low.data_ptr(), 3, ih, iw, oh, ow, 1024, 0, M.data_ptr(), s) == 0
        torch.cuda.synchronize()
        _engine_out[k] = (L.cpu(), M.cpu())
    return _engine_out[k]


def _score(eng, k: int, offset: float, boxes=None, n: int = 3) -> np.ndarray:
    b = None if boxes is None else torch.as_tensor(np.asarray(boxes, dtype=np.float32)).cuda()
    c = eng.score_masks(_low()[:n].contiguous().cuda(), SHAPES[k][0], SHAPES[k][1], offset, boxes=b)
    torch.cuda.synchronize()
    assert c.dtype == torch.int64 and tuple(c.shape) == (n, 4)
    return c.cpu().numpy()


# ---- 1: exact against the engine's own logits ---------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_counts_equal_the_engines_own_logits_and_mask(eng, k, offset):
    L, M = _engine(eng, k)
    got = _score(eng, k, offset)
    want = np.stack([(L > t).flatten(1).sum(1).numpy() for t in (offset, 0.0, -offset)], axis=1)
    print(f"{SHAPE_IDS[k]} offset {offset}: device {got[:, :3].tolist()} from logits {want.tolist()} mask bytes "
          f"{M.flatten(1).sum(1).tolist()}")
    assert np.array_equal(got[:, :3], want)
    assert np.array_equal(got[:, 1], M.flatten(1).sum(1).numpy()), "n_mid is not the number of set bytes of the uint8 mask"
    assert (got[:, 0] <= got[:, 1]).all() and (got[:, 1] <= got[:, 2]).all()
    assert not got[:, 3].any()                                                    # no boxes: n_in = 0
    assert np.array_equal(_score(eng, k, offset, n=1), got[:1])                   # n = 1 and n = 3 give the same rows


def test_offset_zero_gives_three_equal_counts(eng):
    got = _score(eng, 1, 0.0)
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 1], got[:, 2])
    assert np.array_equal(got[:, 1], _engine(eng, 1)[1].flatten(1).sum(1).numpy())


# ---- 2: against the host reference --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_counts_against_the_interpolate_reference(eng, k, offset):
    want, band = quality_ref.counts(_ref(k), offset)
    got = _score(eng, k, offset)
    print(f"{SHAPE_IDS[k]} offset {offset}: |device - reference| {np.abs(got[:, :3] - want[:, :3]).tolist()} band {band.tolist()}")
    assert (band <= 32).all(), f"the reference's own band is wide: {band.tolist()}"        # a wide band cannot hide a wrong kernel
    assert (np.abs(got[:, :3] - want[:, :3]) <= band).all()


# ---- 3: in-box counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_inside_counts_equal_the_host_count_over_the_engines_mask(eng, k):
    _, M = _engine(eng, k)
    h, w = SHAPES[k][1]
    frac = [0.25 * w + 0.5, 0.125 * h + 0.25, 0.75 * w - 0.25, 0.625 * h + 0.75]        # fractional corners
    part = [-10.5, 0.5 * h, 0.5 * w, h + 100.0]                                          # partly outside the image
    full = [0.0, 0.0, w - 1.0, h - 1.0]                                                  # covering the image
    inv = [0.75 * w, 0.75 * h, 0.25 * w - 1.0, 0.25 * h - 1.0]                           # inverted
    for boxes in ([frac, part, full], [inv, full, frac]):
        got = _score(eng, k, 1.0, boxes)
        want = quality_ref.inside_count(M.numpy(), boxes)
        assert np.array_equal(got[:, 3], want), (boxes, got[:, 3].tolist(), want.tolist())
        assert np.array_equal(got[:, :3], _score(eng, k, 1.0)[:, :3])             # the boxes change nothing else
        j = boxes.index(full)
        assert got[j, 3] == got[j, 1]                                             # the whole image: n_in == n_mid
        if inv in boxes:
            assert got[boxes.index(inv), 3] == 0                                  # an inverted box holds nothing
    assert not _score(eng, k, 1.0, None)[:, 3].any()


# ---- 4: constant fields -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 3], ids=[SHAPE_IDS[0], SHAPE_IDS[1], SHAPE_IDS[3]])
def test_constant_fields(eng, k):
    (ih, iw), (oh, ow) = SHAPES[k]
    low = torch.full((2, 256, 256), 5.0, device="cuda")
    c = eng.score_masks(low, (ih, iw), (oh, ow), 1.0).cpu().numpy()
    assert c[:, :3].tolist() == [[oh * ow] * 3] * 2 and quality.stability(c).tolist() == [1.0, 1.0]
    c = eng.score_masks(-low, (ih, iw), (oh, ow), 1.0)
    assert not c.cpu().numpy().any() and quality.stability(c.cpu().numpy()).tolist() == [0.0, 0.0]
    masks = torch.ones(2, oh, ow, dtype=torch.uint8, device="cuda")
    keep = eng.filter_masks(masks, c, min_stability=1e-6)                         # an empty low-threshold mask fails any threshold > 0
    assert keep.cpu().tolist() == [0, 0] and not masks.any()


# ---- 5: reproducibility -------------------------------------------------------------------------------------------------------
def test_two_calls_into_one_buffer_are_bitwise_equal(eng):
    low = _low().cuda()
    boxes = torch.tensor([[10.5, 20.5, 700.0, 500.0]] * 3, device="cuda")
    buf = torch.full((3, 4), -7, dtype=torch.int64, device="cuda")
    out = eng.score_masks(low, *SHAPES[2], 1.0, boxes=boxes, counts_out=buf)
    assert out.data_ptr() == buf.data_ptr()
    first = buf.cpu().numpy().copy()
    eng.score_masks(low, *SHAPES[2], 1.0, boxes=boxes, counts_out=buf)           # overwritten, not accumulated
    assert buf.cpu().numpy().tobytes() == first.tobytes() and (first[:, :3] > 0).all()


# ---- 6: bad arguments ---------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_outputs_untouched(eng):
    from samrs_amd import engine
    lib, h = eng.lib, eng.handle
    low = _low().cuda()
    cnt = torch.full((3, 4), -7, dtype=torch.int64, device="cuda")
    lp, cp = low.data_ptr(), cnt.data_ptr()

    def score(lowres, n, ih, iw, oh, ow, offset, counts=cp):
        rc = lib.samrs_score_masks(h, lowres, n, ih, iw, oh, ow, offset, None, counts, None)
        torch.cuda.synchronize()
        return rc

    for args in ((lp, -1, 1024, 1024, 8, 8, 1.0), (None, 3, 1024, 1024, 8, 8, 1.0), (lp, 3, 1024, 1024, 8, 8, 1.0, None),
                 (lp, 3, 1024, 1024, 8, 8, -1.0), (lp, 3, 1024, 1024, 8, 8, float("nan")), (lp, 3, 1024, 1024, 8, 8, float("inf")),
                 (lp, 3, 0, 1024, 8, 8, 1.0), (lp, 3, 1024, 1025, 8, 8, 1.0), (lp, 3, 512, 512, 8, 8, 1.0), (lp, 3, 1024, 1024, 0, 8, 1.0),
                 (lp, 3, 1024, 1024, 8, -1, 1.0), (lp, 3, 1024, 1024, 46341, 46341, 1.0)):
        assert score(*args) == engine.ERR_BAD_ARG, args
    assert (cnt == -7).all()
    assert score(lp, 0, 1024, 1024, 8, 8, 1.0) == engine.OK and (cnt == -7).all()         # n == 0 is a no-op
    assert score(lp, 3, 1024, 1024, 8, 8, 0.0) == engine.OK and (cnt >= 0).all()

    masks = torch.ones(3, 8, 8, dtype=torch.uint8, device="cuda")
    keep = torch.full((3,), 9, dtype=torch.uint8, device="cuda")
    iou = torch.zeros(3, device="cuda")
    cnt.zero_()                                                                    # every mask would be dropped by min_stability
    mp, kp, ip = masks.data_ptr(), keep.data_ptr(), iou.data_ptr()

    def filt(m, n, hh, ww, c, q, ts, tq, tb, k):
        rc = lib.samrs_filter_masks(h, m, n, hh, ww, c, q, ts, tq, tb, k, None)
        torch.cuda.synchronize()
        return rc

    for args in ((mp, -1, 8, 8, cp, ip, 0.5, 0.0, 0.0, kp), (None, 3, 8, 8, cp, ip, 0.5, 0.0, 0.0, kp), (mp, 3, 8, 8, None, ip, 0.5, 0.0, 0.0, kp),
                 (mp, 3, 8, 8, cp, ip, 0.5, 0.0, 0.0, None), (mp, 3, 0, 8, cp, ip, 0.5, 0.0, 0.0, kp), (mp, 3, 8, 0, cp, ip, 0.5, 0.0, 0.0, kp),
                 (mp, 3, 8, 8, cp, None, 0.0, 0.5, 0.0, kp), (mp, 3, 8, 8, cp, ip, float("nan"), 0.0, 0.0, kp)):
        assert filt(*args) == engine.ERR_BAD_ARG, args
    assert (keep == 9).all() and (masks == 1).all()
    assert filt(mp, 0, 8, 8, cp, ip, 0.5, 0.0, 0.0, kp) == engine.OK and (keep == 9).all() and (masks == 1).all()
    assert filt(mp, 3, 8, 8, cp, None, 0.5, 0.0, 0.0, kp) == engine.OK            # a null iou is fine while its criterion is off
    assert keep.cpu().tolist() == [0, 0, 0] and not masks.any()
    # the Python conventions
    with pytest.raises(ValueError):
        eng.score_masks(low[:, :100], (1024, 1024), (8, 8))
    with pytest.raises(ValueError):
        eng.score_masks(low, (1024, 1024), (8, 8), offset=-1.0)
    with pytest.raises(ValueError):
        eng.score_masks(low, (1024, 1024), (8, 8), boxes=torch.zeros(2, 4, device="cuda"))
    with pytest.raises(ValueError):
        eng.score_masks(low, (1024, 1024), (8, 8), counts_out=torch.zeros(3, 4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        eng.filter_masks(masks, cnt, None, min_pred_iou=0.5)
    with pytest.raises(ValueError):
        eng.filter_masks(masks, cnt[:2])
    assert tuple(eng.score_masks(low[:0].contiguous(), (1024, 1024), (8, 8)).shape) == (0, 4)


# ---- 7: the gate --------------------------------------------------------------------------------------------------------------
ROWS = np.array([[95, 100, 100, 60],        # stability exactly at 0.95f (kept), 0.6 inside
                 [94, 100, 100, 100],       # stability below
                 [99, 100, 100, 100],       # predicted IoU exactly at the threshold (dropped: strict)
                 [0, 0, 0, 0],              # n_lo == 0: the stability test fails; n_mid == 0: the box-fit test passes
                 [0, 0, 5, 0],              # n_mid == 0 with a non-empty low-threshold mask
                 [99, 100, 100, 49]],       # less than half inside its box
                dtype=np.int64)
ROW_IOU = np.array([0.9, 0.9, 0.88, 0.9, 0.9, 0.95], dtype=np.float32)
THRESHOLDS = [(0.95, 0.0, 0.0), (0.0, 0.88, 0.0), (0.0, 0.0, 0.5), (0.95, 0.88, 0.5), (0.0, 0.0, 0.0), (-1.0, -1.0, -1.0), (0.5, 0.0, 0.6)]


@pytest.mark.parametrize("shape,rows", [((5, 67, 93), slice(0, 5)), ((3, 70, 272), slice(0, 3)), ((3, 70, 272), slice(3, 6))])
def test_filter_masks_against_keep_rule(eng, shape, rows):
    n, h, w = shape
    rng = np.random.default_rng(n * w)
    host = (rng.random((n + 1, h, w)) < 0.5).astype(np.uint8)
    host[:, 0, 0] = 1                                                              # no mask starts out empty
    counts, iou = ROWS[rows], ROW_IOU[rows]
    dc, dq = torch.from_numpy(counts).cuda(), torch.from_numpy(iou).cuda()
    for ts, tq, tb in THRESHOLDS:
        buf = torch.from_numpy(host).cuda()
        view = buf[1:]                                                             # the base pointer offset by one mask
        vec = view.data_ptr() % 16 == 0 and (h * w) % 16 == 0
        assert vec == (shape == (3, 70, 272)), "the two shapes must take the two store paths"
        keep = eng.filter_masks(view, dc, dq, ts, tq, tb)
        torch.cuda.synchronize()
        want = quality.keep_rule(counts, iou, ts, tq, tb)
        assert keep.dtype == torch.uint8 and keep.cpu().numpy().astype(bool).tolist() == want.tolist(), (ts, tq, tb)
        got = buf.cpu().numpy()
        assert np.array_equal(got[0], host[0])                                     # the mask in front of the view is not touched
        for j in range(n):
            if want[j]:
                assert got[1 + j].tobytes() == host[1 + j].tobytes(), f"kept mask {j} changed"
            else:
                assert not got[1 + j].any(), f"dropped mask {j} is not all zero"
    # the expectations themselves, so that keep_rule cannot drift with the kernel
    full = quality.keep_rule(ROWS, ROW_IOU, 0.95, 0.88, 0.5).tolist()
    assert full == [True, False, False, False, False, False]
    assert quality.keep_rule(ROWS, ROW_IOU, 0.95).tolist() == [True, False, True, False, False, True]
    assert quality.keep_rule(ROWS, ROW_IOU, 0, 0.88).tolist() == [True, True, False, True, True, True]
    assert quality.keep_rule(ROWS, ROW_IOU, 0, 0, 0.5).tolist() == [True, True, True, True, True, False]
    # a caller-owned slice and a bool view
    tab = torch.full((2, 8), 9, dtype=torch.uint8, device="cuda")
    m = torch.from_numpy(host[1:]).cuda().view(torch.bool)
    out = eng.filter_masks(m, dc, dq, 0.95, 0.88, 0.5, keep_out=tab[1, 2:2 + n])
    assert out.data_ptr() == tab[1, 2:2 + n].data_ptr() and (tab[0] == 9).all() and (tab[1, :2] == 9).all()


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
SIZES = [(1024, 1024), (600, 800)]


def _items(driver):
    items = []
    for i, (h, w) in enumerate(SIZES):
        boxes, labels = synth.make_boxes(60 + i, 4, h, w)
        items.append(driver.WorkItem(f"B{i:04d}", synth.make_image(60 + i, h, w), boxes, labels))
    return items


def _collect(pipe, batches):
    got = {}

    def sink(results, release):
        for r in results:
            r.rles = [r.rle(j) for j in range(len(r.labels))] if r.rle_table is not None else None
            r.seg_mask = None if r.seg_mask is None else r.seg_mask.copy()
            r.masks = None if r.masks is None else r.masks.copy()
            r.rle_data = r.png_data = r.gt_rle_data = None
            got[r.key] = r
        release()

    pipe.run(batches, sink)
    return got


def _host_stability(logits: torch.Tensor, offset: float) -> np.ndarray:
    """fp32 [n, C]: the counts of the full-resolution logits, divided in fp64 (0 / 0 -> 0), rounded once."""
    hi = (logits > offset).flatten(2).sum(2).double()
    lo = (logits > -offset).flatten(2).sum(2).double()
    return torch.where(lo > 0, hi / lo.clamp(min=1), torch.zeros_like(hi)).float().cpu().numpy()


# ---- 8: predictor stability, exact --------------------------------------------------------------------------------------------
def test_predictor_stability_score_equals_the_full_resolution_logits():
    import samrs_amd
    from samrs_amd import driver
    sam = _sam(max_images=1, max_prompts=4)
    pred = samrs_amd.SamPredictor(sam)
    with pytest.raises(RuntimeError, match="An image must be set"):
        pred.stability_score(torch.zeros(1, 1, 256, 256))
    for it, multimask in zip(_items(driver), (True, False)):
        pred.set_image(it.image)
        tb = pred.transform.apply_boxes_torch(torch.from_numpy(it.boxes).cuda(), it.image.shape[:2])
        logits, _, low = pred.predict_torch(None, None, tb, None, multimask_output=multimask, return_logits=True)
        for offset in OFFSETS:
            got = pred.stability_score(low, offset)
            assert got.dtype == torch.float32 and tuple(got.shape) == tuple(low.shape[:2])
            want = _host_stability(logits, offset)
            print(f"{it.key} offset {offset}: stability {got.cpu().numpy().round(4).tolist()}")
            assert got.cpu().numpy().tobytes() == want.tobytes()


# ---- 9: against the oracle ----------------------------------------------------------------------------------------------------
# Largest |stability_engine - stability_oracle| over the fixture's boxes, measured on an MI355X (profiles/quality_parity.txt).
# The bound is twice that: the engine's f16 operands re-roll pixels near the two thresholds (about +-2e-4 IoU).
ORACLE_MEASURED = 4.882e-05          # fixture boxes B0000 / B0001, vit_tiny f16 (split 15), offset 1.0: 4.8816e-05 at box 3 of B0001
ORACLE_TOL = 2 * ORACLE_MEASURED


def test_stability_against_the_oracle():
    import samrs_amd
    from samrs_amd import driver
    from oracle import sam_oracle as so
    cfg = synth.CONFIGS["vit_tiny"]
    sam = _sam(max_images=1, max_prompts=4, precision="f16")
    pred = samrs_amd.SamPredictor(sam)
    orc = so.OraclePredictor(_weights(), cfg)
    worst, rows = 0.0, []
    for it in _items(driver):
        pred.set_image(it.image)
        orc.set_image(it.image)
        tb = pred.transform.apply_boxes_torch(torch.from_numpy(it.boxes).cuda(), it.image.shape[:2])
        _, _, low = pred.predict_torch(None, None, tb, None, multimask_output=False)
        got = pred.stability_score(low, 1.0).cpu().numpy()[:, 0]
        logits, _, _ = orc.predict_torch(None, None, tb.cpu(), None, multimask_output=False, return_logits=True)
        want = quality_ref.stability_score(logits, 0.0, 1.0).numpy()[:, 0]
        d = np.abs(got.astype(np.float64) - want.astype(np.float64))
        rows.append({"image": it.key, "engine": got.tolist(), "oracle": want.tolist(), "abs_diff": d.tolist()})
        worst = max(worst, float(d.max()))
    print("quality_parity " + json.dumps({"max_abs_diff": worst, "rows": rows}))
    assert worst <= ORACLE_TOL, f"largest |stability_engine - stability_oracle| {worst:.3e} > {ORACLE_TOL:.3e}"


# ---- 10: pipeline, quality only -----------------------------------------------------------------------------------------------
PIPE_KW = dict(batch=2, box_batch=3, max_boxes=8, rle=True, rle_buffer_mb=64, keep_masks=True)


@pytest.fixture(scope="module")
def pipe_runs():
    """The fixture batch through TilePipeline with quality off and on (no threshold): computed once, shared by the tests below."""
    from samrs_amd import driver
    sam = _sam(max_images=4, max_prompts=20, precision="f16")
    items = _items(driver)
    p_off = driver.TilePipeline(sam, N_CLASSES, **PIPE_KW)
    off = _collect(p_off, driver.batched(items, 2))
    p_on = driver.TilePipeline(sam, N_CLASSES, quality=True, **PIPE_KW)
    on = _collect(p_on, driver.batched(items, 2))
    torch.cuda.synchronize()
    return dict(sam=sam, items=items, off=off, on=on, p_off=p_off, p_on=p_on)


SAME_FIELDS = ("seg_mask", "areas", "masks", "rle_table")


def test_pipeline_quality_alone_changes_no_output(pipe_runs):
    import samrs_amd
    sam, items, off, on = (pipe_runs[k] for k in ("sam", "items", "off", "on"))
    p_off, p_on = pipe_runs["p_off"], pipe_runs["p_on"]
    assert not hasattr(p_off, "cnt_dev") and not hasattr(p_off, "keep_dev") and not hasattr(p_off, "qual_dev")      # off: nothing allocated
    assert torch.equal(p_off.class_pixels, p_on.class_pixels) and torch.equal(p_off.class_instances, p_on.class_instances)
    pred = samrs_amd.SamPredictor(sam)
    for it in items:
        a, b = on[it.key], off[it.key]
        for f in SAME_FIELDS:
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert a.rles == b.rles
        assert b.score_counts is None and b.kept is None and b.quality is None
        assert a.score_counts.dtype == np.int64 and a.score_counts.shape == (len(it.labels), 4)
        assert np.array_equal(a.score_counts[:, 1], a.areas)
        assert (a.score_counts[:, 0] <= a.score_counts[:, 1]).all() and (a.score_counts[:, 1] <= a.score_counts[:, 2]).all()
        assert np.array_equal(a.score_counts[:, 3], quality_ref.inside_count(a.masks, it.boxes))     # the box as staged: original frame
        assert a.kept.dtype == bool and a.kept.all()
        pred.set_image(it.image)
        tb = pred.transform.apply_boxes_torch(torch.from_numpy(it.boxes).cuda(), it.image.shape[:2])
        _, iou, low = pred.predict_torch(None, None, tb, None, multimask_output=False)
        assert a.quality.dtype == np.float32 and a.quality.tobytes() == iou[:, 0].cpu().numpy().tobytes()
        assert np.array_equal(quality.stability(a.score_counts).astype(np.float32), pred.stability_score(low).cpu().numpy()[:, 0])


# ---- 11: pipeline, with a threshold -------------------------------------------------------------------------------------------
def test_pipeline_threshold_drops_instances_before_they_are_painted(pipe_runs):
    from samrs_amd import driver
    sam, items, on = pipe_runs["sam"], pipe_runs["items"], pipe_runs["on"]
    stab = np.concatenate([quality.stability(on[it.key].score_counts) for it in items])
    thr = float(np.median(stab))
    print(f"stabilities {np.sort(stab).round(4).tolist()} threshold {thr:.6f}")
    runs = {}
    for bd in (False, True):
        p = driver.TilePipeline(sam, N_CLASSES, min_stability=thr, batch_decode=bd, **PIPE_KW)
        assert p.quality and p.filter
        runs[bd] = (_collect(p, driver.batched(items, 2)), p)
    got, p = runs[False]
    n_kept = n_dropped = 0
    pix, ins = np.zeros(N_CLASSES, np.int64), np.zeros(N_CLASSES, np.int64)
    for it in items:
        r, u = got[it.key], on[it.key]
        want = quality.keep_rule(u.score_counts, u.quality, min_stability=thr)
        n_kept, n_dropped = n_kept + int(want.sum()), n_dropped + int((~want).sum())
        assert np.array_equal(r.kept, want)
        assert np.array_equal(r.score_counts, u.score_counts) and r.quality.tobytes() == u.quality.tobytes()
        assert np.array_equal(r.seg_mask, quality_ref.repaint(u.masks, it.labels, want))       # a host repaint of the kept masks
        assert np.array_equal(r.areas, np.where(want, u.areas, 0))                              # dropped areas are 0
        assert np.array_equal(r.masks, u.masks * want[:, None, None].astype(np.uint8))
        for j in np.flatnonzero(want):
            assert r.rles[j] == u.rles[j]
            if u.areas[j] > 0:
                pix[int(it.labels[j])] += int(u.areas[j])
                ins[int(it.labels[j])] += 1
    assert n_kept > 0 and n_dropped > 0, (n_kept, n_dropped)                      # some instances drop and some stay
    assert p.class_pixels.cpu().numpy().tolist() == pix.tolist()                   # the class statistics count the kept instances only
    assert p.class_instances.cpu().numpy().tolist() == ins.tolist()
    other, p2 = runs[True]                                                         # batch_decode: every output identical
    assert torch.equal(p.class_pixels, p2.class_pixels) and torch.equal(p.class_instances, p2.class_instances)
    for it in items:
        a, b = got[it.key], other[it.key]
        for f in SAME_FIELDS + ("score_counts", "kept", "quality"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert a.rles == b.rles


def test_other_thresholds_through_the_pipeline(pipe_runs):
    """min_pred_iou and min_inside_box reach the device rule too: kept == keep_rule on the unfiltered run's counts."""
    from samrs_amd import driver
    sam, items, on = pipe_runs["sam"], pipe_runs["items"], pipe_runs["on"]
    f = float(np.median(np.concatenate([quality.inside_fraction(on[it.key].score_counts) for it in items])))
    q = float(np.median(np.concatenate([on[it.key].quality for it in items])))
    q = q if q > 0 else 0.5            # seeded random weights predict IoUs below 0: any threshold > 0 then drops every instance
    for ts, tq, tb in ((0.0, 0.0, f), (0.0, q, 0.0)):
        got = _collect(driver.TilePipeline(sam, N_CLASSES, min_pred_iou=tq, min_inside_box=tb, **PIPE_KW), driver.batched(items, 2))
        for it in items:
            u = on[it.key]
            want = quality.keep_rule(u.score_counts, u.quality, ts, tq, tb)
            assert np.array_equal(got[it.key].kept, want)
            assert np.array_equal(got[it.key].seg_mask, quality_ref.repaint(u.masks, it.labels, want))


# ---- 12: the CLI and the pipelines that refuse --------------------------------------------------------------------------------
def test_generate_cli_quality_and_min_stability(tmp_path):
    from samrs_amd import driver, generate, tile_io
    items = _items(driver)
    img_dir = tmp_path / "img"
    img_dir.mkdir()
    ann = {}
    for it in items:
        tile_io.write_rgb(str(img_dir / f"{it.key}.png"), it.image, 1)
        ann[it.key] = {"boxes": it.boxes.tolist(), "labels": it.labels.tolist()}
    (tmp_path / "boxes.json").write_text(json.dumps(ann))
    torch.save(_weights(), str(tmp_path / "weights.pth"))
    base = ["--images", str(img_dir), "--boxes", str(tmp_path / "boxes.json"), "--model", "vit_tiny", "--box-batch", "20", "--batch", "2",
            "--checkpoint", str(tmp_path / "weights.pth")]
    generate.main(base + ["--out", str(tmp_path / "off")])
    generate.main(base + ["--out", str(tmp_path / "q"), "--quality"])

    def load(run, key):
        with open(tmp_path / run / "ins" / f"{key}.pkl", "rb") as f:
            return pickle.load(f)

    new = ("pred_iou", "stability", "inside_box")
    stab = []
    for it in items:
        for sub in ("gray", "color"):
            assert open(tmp_path / "q" / sub / f"{it.key}.png", "rb").read() == open(tmp_path / "off" / sub / f"{it.key}.png", "rb").read()
        info, plain = load("q", it.key), load("off", it.key)
        assert len(info) == len(plain) == len(it.labels)
        for e, p in zip(info, plain):
            assert all(type(e[k]) is float for k in new)
            stripped = {k: v for k, v in e.items() if k not in new}
            assert sorted(stripped) == sorted(p)
            assert np.array_equal(stripped["bbox"], p["bbox"]) and all(stripped[k] == p[k] for k in p if k != "bbox")
            stab.append(e["stability"])
    thr = float(np.median(stab))
    log = tmp_path / "run.log"
    generate.main(base + ["--out", str(tmp_path / "f"), "--min-stability", repr(thr), "--log", str(log)])
    thr32 = float(np.float32(thr))
    n_dropped = 0
    for it in items:
        info, full = load("f", it.key), load("q", it.key)
        kept = [e for e in full if e["stability"] >= thr32]
        n_dropped += len(full) - len(kept)
        assert [e["label"] for e in info] == [e["label"] for e in kept] and [e["mask"] for e in info] == [e["mask"] for e in kept]
        assert [e["stability"] for e in info] == [e["stability"] for e in kept]
    assert 0 < n_dropped < len(stab)
    lines = [json.loads(l) for l in open(log).read().splitlines()]
    batches = [l for l in lines if "images" in l]
    assert sum(sum(l["dropped"]) for l in batches) == n_dropped and batches[-1]["dropped_total"] == n_dropped
    cs = json.load(open(tmp_path / "f" / "statistic" / "class_stats.json"))
    assert cs["quality"]["dropped_instance_num"] == n_dropped and cs["quality"]["min_stability"] == thr
    assert "quality" not in json.load(open(tmp_path / "off" / "statistic" / "class_stats.json"))


def test_instance_and_scene_pipelines_refuse_the_options():
    from samrs_amd import driver
    from samrs_amd.scene import ScenePipeline
    sam = _sam(max_images=4, max_prompts=6)
    with pytest.raises(ValueError, match="quality"):
        driver.InstancePipeline(sam, 1, quality=True, batch=2)
    with pytest.raises(ValueError, match="min_stability"):
        ScenePipeline(sam, N_CLASSES, window=256, overlap=64, min_stability=0.9)
    driver.InstancePipeline(sam, 1, quality=False, batch=2)                        # the defaults pass through
