"""GPU: samrs_resolve_overlaps (overlap_kernels.hip) alone, then the stage through TilePipeline and the generation CLI.

Kernel level (vit_tiny engine): the logits are the engine's own fp32 output of samrs_k_postprocess for quality_ref.make_low(4, 3) on
the five quality_ref.SHAPES, as tests/test_quality_gpu.py obtains them; the reference is tests/overlap_ref.py on those logits.  Three
mask sets: L > 0 (dense: most pixels contested), L > 6 (sparse: the uncontested fast path) and masks[j] = L[(j + 1) % n] > 2 (the
gate is independent of the mask's own logit: negative logits compete).  Rule LOGIT is compared outside the band -- the contested
pixels whose two best candidates' logits differ by <= quality_ref.LOGIT_TOL -- after asserting that the band holds <= 32 pixels;
the mismatch count is printed and expected to be 0, because postprocess_kernel and overlap_resolve_kernel expand the same macro.
Rules SMALLEST and PRIORITY without logits are integer-only and compared exactly."""
import functools
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from samrs_amd import rle as rle_mod
from samrs_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import overlap_ref  # noqa: E402
import quality_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N_CLASSES = 18
SHAPES = quality_ref.SHAPES
SHAPE_IDS = [f"{a[0]}x{a[1]}-{b[0]}x{b[1]}" for a, b in SHAPES]
TOL = quality_ref.LOGIT_TOL
SETS = ("dense", "sparse", "shifted")
BAND_MAX = 32


@functools.lru_cache(maxsize=None)
def _weights():
    return synth.make_state_dict(synth.CONFIGS["vit_tiny"], 0, logit_scale=synth.MARGIN_LOGIT_SCALE)


def _sam(**kw):
    import samrs_amd
    return samrs_amd.sam_model_registry["vit_tiny"](state_dict=_weights(), **kw).to("cuda")


@pytest.fixture(scope="module")
def eng():
    sam = _sam(max_images=1, max_prompts=4)
    yield sam.engine


@functools.lru_cache(maxsize=None)
def _low(n: int = 4, seed: int = 3):
    return quality_ref.make_low(n, seed)


_logit_cache = {}


def _logits(eng, k: int, n: int = 4, seed: int = 3) -> np.ndarray:
    """fp32 [n, H, W]: the engine's own postprocess output for shape k, on the host; computed once and shared."""
    key = (k, n, seed)
    if key not in _logit_cache:
        (ih, iw), (oh, ow) = SHAPES[k]
        low = _low(n, seed).cuda()
        L = torch.empty(n, oh, ow, dtype=torch.float32, device="cuda")
        assert eng.lib.samrs_k_postprocess(low.data_ptr(), n, ih, iw, oh, ow, 1024, 1, L.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        _logit_cache[key] = L.cpu().numpy()
    return _logit_cache[key]


def _mask_set(L: np.ndarray, kind: str) -> np.ndarray:
    if kind == "dense":
        return (L > 0).astype(np.uint8)
    if kind == "sparse":
        return (L > 6).astype(np.uint8)
    return (np.roll(L, -1, axis=0) > 2).astype(np.uint8) * 255        # masks[j] = L[(j + 1) % n] > 2, as 0 / 255


def _run(eng, masks: np.ndarray, rule, k=None, low=None, priority=None, odd_base: bool = False):
    """One call on a fresh device copy -> (masks, owner, before, removed) on the host."""
    n, h, w = masks.shape
    if odd_base:
        buf = torch.zeros(masks.size + 1, dtype=torch.uint8, device="cuda")
        m = buf[1:].view(n, h, w)
        m.copy_(torch.from_numpy(masks))
        assert m.data_ptr() % 2 == 1
    else:
        m = torch.from_numpy(masks).cuda()
    kw = {}
    if low is not None:
        kw = dict(low=low.cuda(), input_size=SHAPES[k][0], original_size=(h, w))
    if priority is not None:
        kw["priority"] = torch.as_tensor(np.asarray(priority, dtype=np.int64)).cuda()
    out, owner, before, removed = eng.resolve_overlaps(m, rule, **kw)
    torch.cuda.synchronize()
    assert out.data_ptr() == m.data_ptr()
    assert owner.dtype == torch.int32 and tuple(owner.shape) == (h, w) and before.dtype == removed.dtype == torch.int64
    return m.cpu().numpy(), owner.cpu().numpy(), before.cpu().numpy(), removed.cpu().numpy()


def _check_partition(src: np.ndarray, got: np.ndarray, owner: np.ndarray, before: np.ndarray, removed: np.ndarray) -> None:
    """What holds for every rule: the counts are the host popcounts, the masks are pairwise disjoint, their union is the input's
    union, winners keep their byte, and the owner map names the one mask set at each pixel."""
    pop = lambda a: (a != 0).sum(axis=(1, 2)).astype(np.int64)
    assert np.array_equal(before, pop(src))
    assert np.array_equal(before - removed, pop(got))
    cover = (got != 0).sum(0)
    assert cover.max(initial=0) <= 1, "two masks still share a pixel"
    assert np.array_equal(cover > 0, (src != 0).any(0)), "the union changed"
    assert np.array_equal(got[got != 0], src[got != 0]), "a winner's byte was rewritten"
    want_owner = np.where(cover > 0, (got != 0).argmax(0), -1)
    assert np.array_equal(owner, want_owner)


# ---- 1: rule LOGIT against the reference, outside the band --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_logit_rule_equals_the_reference_outside_the_band(eng, k, kind):
    L = _logits(eng, k)
    src = _mask_set(L, kind)
    band = overlap_ref.band(src, L, TOL)
    contested = int(((src != 0).sum(0) >= 2).sum())
    assert band.sum() <= BAND_MAX, f"the band is wide: {int(band.sum())} pixels"     # a wide band cannot hide a wrong kernel
    want, want_owner, want_before, want_removed = overlap_ref.resolve(src, L, overlap_ref.primary(src, "logit"))
    got, owner, before, removed = _run(eng, src, "logit", k, _low())
    miss_m = (got != want).any(0)
    miss_o = owner != want_owner
    print(f"{SHAPE_IDS[k]} {kind}: {contested} of {L[0].size} pixels contested, band {int(band.sum())}, mismatches masks "
          f"{int(miss_m.sum())} owner {int(miss_o.sum())} (expected 0), removed {removed.tolist()}")
    assert not (miss_m & ~band).any() and not (miss_o & ~band).any()
    _check_partition(src, got, owner, before, removed)
    assert np.array_equal(before, want_before)
    assert (np.abs(removed - want_removed) <= int((miss_m | miss_o).sum())).all()       # equal but for the band's pixels
    if k < 3 and kind == "dense":
        assert contested > 0.5 * L[0].size                                               # the set is what it claims to be
    if k < 3 and kind == "sparse":
        assert 0 < contested < 0.1 * L[0].size


# ---- 2: the integer rules, exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", ["smallest", "priority"])
@pytest.mark.parametrize("k", range(len(SHAPES)), ids=SHAPE_IDS)
def test_integer_rules_are_exact(eng, k, rule):
    src = _mask_set(_logits(eng, k), "dense")
    prio = [3, -5, 3, 0] if rule == "priority" else None                                 # two equal keys: the later mask wins there
    want, want_owner, want_before, want_removed = overlap_ref.resolve(src, None, overlap_ref.primary(src, rule, prio))
    got, owner, before, removed = _run(eng, src, rule, priority=prio)
    assert np.array_equal(got, want) and np.array_equal(owner, want_owner)
    assert np.array_equal(before, want_before) and np.array_equal(removed, want_removed)
    _check_partition(src, got, owner, before, removed)


def test_smallest_with_equal_areas_falls_to_the_logit(eng):
    k = 3
    L = _logits(eng, k)
    src = _mask_set(L, "dense")
    src[2] = src[0]                                                                      # equal areas: masks 0 and 2 tie on the key
    P = overlap_ref.primary(src, "smallest")
    assert P[0] == P[2]
    band = overlap_ref.band(src, L, TOL, any_pair=True)
    assert band.sum() <= BAND_MAX
    want, want_owner, _, _ = overlap_ref.resolve(src, L, P)
    got, owner, before, removed = _run(eng, src, "smallest", k, _low())
    assert not ((got != want).any(0) & ~band).any() and not ((owner != want_owner) & ~band).any()
    _check_partition(src, got, owner, before, removed)
    both = (src[0] != 0) & (src[1] == 0) & (src[3] == 0)                                 # pixels only the two tied masks compete for
    assert (owner[both] == np.where(L[2][both] < L[0][both], 0, 2))[~band[both]].all()


# ---- 3: the byte path, more than one counter chunk ------------------------------------------------------------------------------
def test_seventy_masks_at_an_odd_base_address(eng):
    k, n = 3, 70                                                                         # 67 x 93: w % 16 != 0; 70 > one chunk of 64 masks
    low = _low(n, 5)
    L = _logits(eng, k, n, 5)
    src = _mask_set(L, "dense")
    band = overlap_ref.band(src, L, TOL)
    assert band.sum() <= BAND_MAX
    want, want_owner, _, want_removed = overlap_ref.resolve(src, L, None)
    got, owner, before, removed = _run(eng, src, "logit", k, low, odd_base=True)
    miss = (got != want).any(0) | (owner != want_owner)
    print(f"n = 70: band {int(band.sum())}, mismatches {int(miss.sum())} (expected 0)")
    assert not (miss & ~band).any()
    _check_partition(src, got, owner, before, removed)
    assert (np.abs(removed - want_removed) <= int(miss.sum())).all() and removed[64:].sum() > 0
    want, want_owner, want_before, want_removed = overlap_ref.resolve(src, None, overlap_ref.primary(src, "smallest"))
    got, owner, before, removed = _run(eng, src, "smallest", odd_base=True)
    assert np.array_equal(got, want) and np.array_equal(owner, want_owner)
    assert np.array_equal(before, want_before) and np.array_equal(removed, want_removed)


@pytest.mark.parametrize("shape", [(3, 5, 32), (5, 7, 48), (3, 9, 17)])
def test_odd_base_with_rows_of_whole_vectors_and_a_ragged_row(eng, shape):
    """w % 16 == 0 at an odd base address takes the byte path too; 17 = one whole group of 16 and a one-pixel tail."""
    n, h, w = shape
    rng = np.random.default_rng(w)
    src = (rng.random(shape) < 0.6).astype(np.uint8) * 255
    prio = rng.integers(-2, 3, n)
    for odd in (True, False):
        want, want_owner, want_before, want_removed = overlap_ref.resolve(src, None, overlap_ref.primary(src, "priority", prio))
        got, owner, before, removed = _run(eng, src, "priority", priority=prio, odd_base=odd)
        assert np.array_equal(got, want) and np.array_equal(owner, want_owner)
        assert np.array_equal(before, want_before) and np.array_equal(removed, want_removed)


# ---- 4: n = 1, n = 0 ------------------------------------------------------------------------------------------------------------
def test_one_mask_changes_nothing_and_fills_the_outputs(eng):
    k = 1
    L = _logits(eng, k)
    src = _mask_set(L, "shifted")[:1].copy()
    for rule, kw in (("logit", dict(k=k, low=_low()[:1].contiguous())), ("smallest", {}), ("priority", dict(priority=[4]))):
        got, owner, before, removed = _run(eng, src, rule, **kw)
        assert got.tobytes() == src.tobytes()
        assert np.array_equal(owner, np.where(src[0] != 0, 0, -1))
        assert before.tolist() == [int((src != 0).sum())] and removed.tolist() == [0]


def test_no_masks_is_a_no_op(eng):
    from samrs_amd import engine
    m = torch.zeros(0, 8, 8, dtype=torch.uint8, device="cuda")
    out, owner, before, removed = eng.resolve_overlaps(m, "smallest")
    assert (owner == -1).all() and tuple(before.shape) == tuple(removed.shape) == (0,)
    one = torch.ones(1, 8, 8, dtype=torch.uint8, device="cuda")
    own = torch.full((8, 8), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    rc = eng.lib.samrs_resolve_overlaps(eng.handle, one.data_ptr(), 0, 8, 8, 2, None, 0, 0, None, own.data_ptr(), cnt.data_ptr(),
                                        cnt[1:].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == engine.OK and (own == -7).all() and (cnt == -7).all() and (one == 1).all()


# ---- 5: bad arguments -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(eng):
    from samrs_amd import engine
    lib, h = eng.lib, eng.handle
    masks = torch.ones(3, 8, 8, dtype=torch.uint8, device="cuda")
    low = _low().cuda()
    prio = torch.zeros(3, dtype=torch.int64, device="cuda")
    own = torch.full((8, 8), -7, dtype=torch.int32, device="cuda")
    bef = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    rem = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    mp, lp, pp = masks.data_ptr(), low.data_ptr(), prio.data_ptr()

    def call(m, n, hh, ww, rule, lowres, ih, iw, pr):
        rc = lib.samrs_resolve_overlaps(h, m, n, hh, ww, rule, lowres, ih, iw, pr, own.data_ptr(), bef.data_ptr(), rem.data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    for args in ((mp, -1, 8, 8, 1, lp, 1024, 1024, None),              # n < 0
                 (None, 3, 8, 8, 1, lp, 1024, 1024, None),             # null masks
                 (mp, 3, 8, 8, 0, lp, 1024, 1024, pp),                 # unknown rules
                 (mp, 3, 8, 8, 4, lp, 1024, 1024, pp),
                 (mp, 3, 8, 8, 1, None, 1024, 1024, None),             # LOGIT without lowres
                 (mp, 3, 8, 8, 3, lp, 1024, 1024, None),               # PRIORITY without priority
                 (mp, 3, 0, 8, 2, None, 0, 0, None),                   # bad sizes
                 (mp, 3, 8, -1, 2, None, 0, 0, None),
                 (mp, 3, 8, 8, 1, lp, 0, 1024, None),                  # bad input frames, read because lowres is given
                 (mp, 3, 8, 8, 1, lp, 1024, 1025, None),
                 (mp, 3, 8, 8, 2, lp, 512, 512, None),
                 (mp, 3, 46341, 46341, 2, None, 0, 0, None)):          # h * w >= 2^31
        assert call(*args) == engine.ERR_BAD_ARG, args
    assert (own == -7).all() and (bef == -7).all() and (rem == -7).all() and (masks == 1).all()
    assert call(mp, 3, 8, 8, 2, None, 0, 0, None) == engine.OK                          # the input frame is not read without lowres
    assert bef.cpu().tolist() == [64, 64, 64] and rem.cpu().tolist() == [64, 64, 0] and (own == 2).all()
    # the Python conventions
    with pytest.raises(ValueError, match="rule"):
        eng.resolve_overlaps(masks, "nearest")
    with pytest.raises(ValueError, match="low"):
        eng.resolve_overlaps(masks, "logit")
    with pytest.raises(ValueError, match="priority"):
        eng.resolve_overlaps(masks, "priority")
    with pytest.raises(ValueError, match="input_size"):
        eng.resolve_overlaps(masks, "logit", low=low[:3].contiguous())
    with pytest.raises(ValueError, match="original_size"):
        eng.resolve_overlaps(masks, "smallest", original_size=(8, 9))
    with pytest.raises(ValueError, match="owner_out"):
        eng.resolve_overlaps(masks, "smallest", owner_out=torch.zeros(8, 8, dtype=torch.int64, device="cuda"))
    m2 = torch.ones(3, 8, 8, dtype=torch.uint8, device="cuda")
    tab = torch.full((2, 5), -7, dtype=torch.int64, device="cuda")
    _, o, b, r = eng.resolve_overlaps(m2, "smallest", owner_out=False, before_out=False, removed_out=tab[1, 1:4])     # scratch for the areas
    assert o is None and b is None and r.data_ptr() == tab[1, 1:4].data_ptr()
    assert tab.cpu().tolist() == [[-7] * 5, [-7, 64, 64, 0, -7]]


# ---- 6: reproducibility ---------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(eng):
    k = 2
    src = _mask_set(_logits(eng, k), "dense")
    a = _run(eng, src, "logit", k, _low())
    b = _run(eng, src, "logit", k, _low())
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


# ---- 7: permutation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3], ids=[SHAPE_IDS[1], SHAPE_IDS[3]])
def test_permuting_the_masks_permutes_the_owner_and_keeps_the_class_map(eng, k):
    L = _logits(eng, k)
    src = _mask_set(L, "shifted")
    labels = np.array([3, 7, 11, 5])
    idx = np.array([2, 0, 3, 1])
    band = overlap_ref.band(src, L, TOL)
    assert band.sum() <= BAND_MAX
    got, owner, _, removed = _run(eng, src, "logit", k, _low())
    got_p, owner_p, _, removed_p = _run(eng, src[idx], "logit", k, _low()[idx].contiguous())
    back = np.where(owner_p >= 0, idx[np.clip(owner_p, 0, None)], -1)
    assert np.array_equal(back[~band], owner[~band])
    seg, seg_p = overlap_ref.paint(got, labels), overlap_ref.paint(got_p, labels[idx])
    assert np.array_equal(seg[~band], seg_p[~band])
    assert (np.abs(removed[idx] - removed_p) <= int(band.sum())).all()
    assert not np.array_equal(overlap_ref.paint(src, labels), overlap_ref.paint(src[idx], labels[idx]))   # the order rule does depend on it
    # distinct priorities, no logits: exact everywhere
    prio = np.array([5, -1, 9, 2])
    _, own_a, _, _ = _run(eng, src, "priority", priority=prio)
    _, own_b, _, _ = _run(eng, src[idx], "priority", priority=prio[idx])
    assert np.array_equal(np.where(own_b >= 0, idx[np.clip(own_b, 0, None)], -1), own_a)


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
SIZES = [(1024, 1024), (600, 801)]
PIPE_KW = dict(batch=2, box_batch=3, max_boxes=8, rle=True, rle_buffer_mb=64, keep_masks=True, mask_boxes=True)


def _overlapping_boxes(h: int, w: int, seed: int):
    """Six boxes around the image centre, each shifted by a fraction of its size: every box overlaps its neighbours."""
    rng = np.random.default_rng(seed)
    boxes = []
    for j in range(6):
        bw, bh = 0.3 * w + 0.05 * w * (j % 3), 0.3 * h + 0.04 * h * (j % 2)
        cx, cy = 0.5 * w + 0.08 * w * (j - 2.5), 0.5 * h + 0.06 * h * ((j * 2) % 5 - 2)
        boxes.append([max(0.0, cx - bw / 2), max(0.0, cy - bh / 2), min(w - 1.0, cx + bw / 2), min(h - 1.0, cy + bh / 2)])
    return np.asarray(boxes, dtype=np.float32), rng.integers(0, N_CLASSES, 6).astype(np.int64)


def _items(driver):
    items = []
    for i, (h, w) in enumerate(SIZES):
        boxes, labels = _overlapping_boxes(h, w, 70 + i)
        items.append(driver.WorkItem(f"V{i:04d}", synth.make_image(70 + i, h, w), boxes, labels))
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


@pytest.fixture(scope="module")
def world():
    """The fixture batch's masks and logits from SamPredictor, computed once; the sam is shared by the pipelines below."""
    import samrs_amd
    from samrs_amd import driver
    sam = _sam(max_images=4, max_prompts=20, precision="f16")
    items = _items(driver)
    pred = samrs_amd.SamPredictor(sam)
    plain = {}
    for it in items:
        pred.set_image(it.image)
        tb = pred.transform.apply_boxes_torch(torch.from_numpy(it.boxes).cuda(), it.image.shape[:2])
        masks, _, low = pred.predict_torch(None, None, tb, None, multimask_output=False)
        plain[it.key] = (masks[:, 0].contiguous(), low.contiguous(), pred.input_size)
    torch.cuda.synchronize()
    return dict(sam=sam, items=items, plain=plain)


def _hbox(mask: np.ndarray):
    ys, xs = np.nonzero(mask)
    return [int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())] if len(ys) else [0, 0, 0, 0]


@pytest.mark.parametrize("batch_decode", [False, True], ids=["per-tile", "batch-decode"])
@pytest.mark.parametrize("rule", ["logit", "smallest"])
def test_pipeline_outputs_are_those_of_the_disjoint_masks(world, rule, batch_decode):
    from samrs_amd import driver
    sam, items, plain = world["sam"], world["items"], world["plain"]
    p = driver.TilePipeline(sam, N_CLASSES, overlap=rule, batch_decode=batch_decode, **PIPE_KW)
    got = _collect(p, driver.batched(items, 2))
    pix, ins = np.zeros(N_CLASSES, np.int64), np.zeros(N_CLASSES, np.int64)
    for it in items:
        r = got[it.key]
        masks, low, in_size = plain[it.key]
        src = masks.view(torch.uint8).cpu().numpy()
        want, _, before, removed = sam.engine.resolve_overlaps(masks.clone(), rule, low=low, input_size=in_size,
                                                               original_size=it.image.shape[:2], owner_out=False)
        want = want.view(torch.uint8).cpu().numpy()
        print(f"{it.key} {rule}: before {before.cpu().tolist()} removed {removed.cpu().tolist()}")
        assert int(removed.sum()) > 0, "the fixture's masks do not overlap: the test shows nothing"
        assert ((want != 0).sum(0) <= 1).all() and np.array_equal((want != 0).any(0), (src != 0).any(0))
        assert np.array_equal(r.masks, want)                                             # the kept masks are the resolved ones
        assert np.array_equal(r.removed, removed.cpu().numpy()) and r.removed.dtype == np.int64
        assert np.array_equal(r.areas, (want != 0).sum(axis=(1, 2)))
        assert np.array_equal(r.seg_mask, overlap_ref.paint(want, it.labels))
        for j in range(len(it.labels)):
            assert np.array_equal(rle_mod.decode(r.rles[j]), want[j] != 0)
            if r.areas[j]:
                assert r.mask_hbox[j].tolist() == _hbox(want[j])
                pix[int(it.labels[j])] += int(r.areas[j])
                ins[int(it.labels[j])] += 1
            else:
                assert r.mask_record[j, 6] == 0
        # disjoint masks: the class map is the same whatever order they are painted in
        assert np.array_equal(r.seg_mask, overlap_ref.paint(want[::-1], it.labels[::-1]))
    assert p.class_pixels.cpu().numpy().tolist() == pix.tolist() and p.class_instances.cpu().numpy().tolist() == ins.tolist()


def test_pipeline_order_is_the_pipeline_without_the_argument(world):
    from samrs_amd import driver
    sam, items = world["sam"], world["items"]
    p_plain = driver.TilePipeline(sam, N_CLASSES, **PIPE_KW)
    p_order = driver.TilePipeline(sam, N_CLASSES, overlap="order", **PIPE_KW)
    assert not hasattr(p_order, "rem_dev") and [t.field for t in p_order.tables] == [t.field for t in p_plain.tables]
    a, b = _collect(p_plain, driver.batched(items, 2)), _collect(p_order, driver.batched(items, 2))
    import dataclasses
    for it in items:
        for f in dataclasses.fields(driver.TileResult):
            x, y = getattr(a[it.key], f.name), getattr(b[it.key], f.name)
            if isinstance(x, np.ndarray):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), f.name
            else:
                assert (x is None and y is None) or x == y, f.name
        assert a[it.key].rles == b[it.key].rles and a[it.key].removed is None
        src = a[it.key].masks
        assert ((src != 0).sum(0) >= 2).any()                                            # "order" leaves the overlaps in place
    with pytest.raises(ValueError, match="overlap"):
        driver.TilePipeline(sam, N_CLASSES, overlap="priority", **PIPE_KW)


def test_generate_cli_overlap(tmp_path):
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
    generate.main(base + ["--out", str(tmp_path / "on"), "--overlap", "logit"])

    def load(run, key):
        with open(tmp_path / run / "ins" / f"{key}.pkl", "rb") as f:
            return pickle.load(f)

    total = 0
    for it in items:
        info, plain = load("on", it.key), load("off", it.key)
        assert len(info) == len(plain) == len(it.labels)
        assert all("removed" not in e for e in plain) and all(type(e["removed"]) is int for e in info)
        dec = np.stack([rle_mod.decode(e["mask"]) for e in info])
        old = np.stack([rle_mod.decode(e["mask"]) for e in plain])
        assert (dec.sum(0) <= 1).all() and np.array_equal(dec.any(0), old.any(0))       # disjoint, same union
        assert (old.sum(0) >= 2).any()
        for e, o, d, q in zip(info, plain, dec, old):
            assert e["size"] == int(d.sum()) and e["removed"] == int(q.sum()) - int(d.sum())
            assert sorted(k for k in e if k != "removed") == sorted(o)
        total += sum(e["removed"] for e in info)
    cs = json.load(open(tmp_path / "on" / "statistic" / "class_stats.json"))
    assert cs["overlap"]["rule"] == "logit" and cs["overlap"]["removed_pixel_num"] == total and total > 0
    assert "overlap" not in json.load(open(tmp_path / "off" / "statistic" / "class_stats.json"))
    with pytest.raises(SystemExit):
        generate.main(base + ["--out", str(tmp_path / "x"), "--overlap", "logit", "--scene-window", "512"])
