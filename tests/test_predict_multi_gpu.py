"""GPU: samrs_predict_multi (Engine.predict_multi) -- the prompts of several images in one decoder chain -- against a loop of
Engine.predict over the same slots.  The multi-image call only changes where each prompt reads its image side, so every
output must match byte for byte: masks, IoU, low-res logits and the fp32 logits of return_logits."""
import ctypes

import numpy as np
import pytest
import torch

from samrs_amd import synth

pytestmark = pytest.mark.gpu

# (input size, original size) of the three test images: square, square shown smaller, ragged
IMAGES = [((1024, 1024), (1024, 1024)), ((1024, 1024), (800, 800)), ((600, 1024), (600, 1024))]
_ENGINES = {}


def _engine(name, max_prompts=64):
    """Engine with IMAGES encoded in slots 0..2 (slot 3 stays unset).  "<model>:unfused": decoder_fusion = 0, the un-fused
    image -> token path that runs the shared layer 0 once per image segment."""
    key = (name, max_prompts)
    if key not in _ENGINES:
        import samrs_amd
        model, _, variant = name.partition(":")
        opts = {"decoder_fusion": 0} if variant == "unfused" else None
        sam = samrs_amd.sam_model_registry[model](precision="f16", max_images=4, max_prompts=max_prompts, max_points=4,
                                                  options=opts).to("cuda")
        tiles = [torch.from_numpy(synth.make_image(40 + i, *ins)).cuda() for i, (ins, _) in enumerate(IMAGES)]
        sam.engine.set_images_ragged(tiles, slot0=0)
        _ENGINES[key] = sam.engine
    return _ENGINES[key]


def _prompts(kind, n, seed, hw=(1024, 1024)):
    """Prompt tensors (boxes, point_coords, point_labels, mask_input) of `n` prompts in the input frame `hw`."""
    rng = np.random.default_rng(seed)
    h, w = hw
    boxes = pc = pl = mi = None
    if "box" in kind:
        boxes = torch.from_numpy(synth.make_boxes(seed, n, h, w)[0]).cuda()
    if "pt" in kind:
        k = 3 if "pt3" in kind else 1
        pc = torch.from_numpy(np.stack([rng.uniform(0, w, (n, k)), rng.uniform(0, h, (n, k))], -1).astype(np.float32)).cuda()
        lab = rng.integers(0, 2, (n, k))
        lab[:, 0] = 1
        if k > 1:
            lab[:, 1] = 0                                       # a background point in every prompt
        pl = torch.from_numpy(lab.astype(np.int32)).cuda()
    if "mask" in kind:
        mi = torch.from_numpy(rng.normal(0, 4, (n, 1, 256, 256)).astype(np.float32)).cuda()
    return boxes, pc, pl, mi


def _cat(parts):
    return None if parts[0] is None else torch.cat(parts)


def _same(a, b):
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    elif a.dtype == torch.bool:
        a, b = a.view(torch.uint8), b.view(torch.uint8)
    assert torch.equal(a, b)


def _check(eng, slots, counts, kind, multimask, return_logits=False, seed=0):
    """predict_multi over (slots, counts) == predict per image, byte for byte."""
    sizes = [IMAGES[s] for s in slots]
    per = [_prompts(kind, n, seed + 7 * i, sizes[i][0]) for i, n in enumerate(counts)]
    args = [_cat([p[j] for p in per]) for j in range(4)]
    masks, iou, low = eng.predict_multi(slots, counts, *args, multimask, return_logits, [s[0] for s in sizes],
                                        [s[1] for s in sizes])
    assert len(masks) == len(iou) == len(low) == len(slots)
    c = 3 if multimask else 1
    for i, (s, n) in enumerate(zip(slots, counts)):
        oh, ow = sizes[i][1]
        assert tuple(masks[i].shape) == (n, c, oh, ow) and tuple(iou[i].shape) == (n, c) and tuple(low[i].shape) == (n, c, 256, 256)
        if n == 0:
            continue
        m0, q0, l0 = eng.predict(s, *per[i], multimask, return_logits, sizes[i][0], sizes[i][1])
        _same(masks[i], m0)
        _same(iou[i], q0)
        _same(low[i], l0)
    torch.cuda.synchronize()


KINDS = ["box", "pt1", "pt3", "mask", "box_pt1", "box_mask"]
MODELS = ["vit_tiny", "vit_tiny80", "vit_tiny80:unfused"]


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("multimask", [False, True])
def test_multi_equals_per_image_loop(name, kind, multimask):
    eng = _engine(name)
    _check(eng, [0, 1, 2], [5, 3, 4], kind, multimask, seed=2 * KINDS.index(kind) + int(multimask))


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("kind", ["box", "pt3", "box_mask"])
def test_return_logits(name, kind):
    _check(_engine(name), [2, 0, 1], [2, 4, 3], kind, True, return_logits=True, seed=11)


@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("kind", ["box", "mask"])
def test_chunk_boundaries_inside_images(name, kind):
    """max_prompts = 5: chunks of 5 prompts cross the image boundaries at 3 and 7 and split the third image."""
    _check(_engine(name, max_prompts=5), [0, 1, 2], [3, 4, 6], kind, True, seed=3)
    _check(_engine(name, max_prompts=5), [2, 2, 0], [6, 5, 1], kind, False, seed=4)


@pytest.mark.parametrize("name", MODELS)
def test_repeated_reversed_sparse_slots_and_empty_images(name):
    eng = _engine(name)
    _check(eng, [2, 0, 2, 1], [2, 3, 0, 4], "box", True, seed=5)
    _check(eng, [2, 1, 0], [1, 1, 1], "pt1", False, seed=6)
    _check(eng, [0, 2], [0, 3], "box_pt1", True, seed=7)
    _check(eng, [2, 0], [4, 4], "box_mask", False, seed=8)


@pytest.mark.parametrize("name", MODELS)
def test_one_image_equals_predict(name):
    eng = _engine(name)
    for s in range(3):
        _check(eng, [s], [6], "box", True, seed=9 + s)
        _check(eng, [s], [2], "mask", False, seed=19 + s)


def test_errors():
    from samrs_amd.engine import ERR_BAD_ARG, PREDICT_MULTI_ARGTYPES
    eng = _engine("vit_tiny")
    b, _, _, _ = _prompts("box", 4, 0)
    with pytest.raises(RuntimeError, match="slot 3 is not set"):
        eng.predict_multi([0, 3], [2, 2], b, None, None, None, False, False, [(1024, 1024)] * 2, [(1024, 1024)] * 2)
    with pytest.raises(ValueError, match="sum to 5"):
        eng.predict_multi([0, 1], [2, 3], b, None, None, None, False, False, [(1024, 1024)] * 2, [(1024, 1024)] * 2)
    with pytest.raises(ValueError, match="2 slots but 1 prompt counts"):
        eng.predict_multi([0, 1], [4], b, None, None, None, False, False, [(1024, 1024)] * 2, [(1024, 1024)] * 2)
    with pytest.raises(ValueError, match="boxes must be Bx4"):
        eng.predict_multi([0], [3], b[:, :3], None, None, None, False, False, [(1024, 1024)], [(1024, 1024)])
    with pytest.raises(AssertionError, match="bad input/original size"):
        eng.predict_multi([0, 1], [2, 2], b, None, None, None, False, False, [(1024, 1024), (1025, 1024)], [(1024, 1024)] * 2)
    # the C entry point itself: offsets that decrease or do not start at 0
    lib = eng.lib
    assert lib.samrs_predict_multi.argtypes == PREDICT_MULTI_ARGTYPES
    ia = ctypes.c_int
    iou = torch.empty(4, 1, device="cuda")
    for offs in ([0, 3, 2], [1, 2, 4]):
        rc = lib.samrs_predict_multi(eng.handle, 2, (ia * 2)(0, 1), (ia * 3)(*offs), b.data_ptr(), None, None, 0, None, 0, 0,
                                     (ia * 4)(1024, 1024, 1024, 1024), (ia * 4)(1024, 1024, 1024, 1024), None, iou.data_ptr(),
                                     None, torch.cuda.current_stream().cuda_stream)
        assert rc == ERR_BAD_ARG and b"prompt_offsets" in lib.samrs_last_error(eng.handle)
    torch.cuda.synchronize()


def test_vit_h_multi_and_per_slot_grade():
    """ViT-H (the fused i2t path at 64 x 64 tokens, multimask grade on): byte-identical with the per-image loop, and the
    multimask precision grade is checked per slot."""
    import samrs_amd
    from samrs_amd.engine import PrecisionError
    sam = samrs_amd.sam_model_registry["vit_h"](precision="f16", max_images=3, max_prompts=8, max_points=1).to("cuda")
    eng = sam.engine
    tiles = [torch.from_numpy(synth.make_image(40 + i, *ins)).cuda() for i, (ins, _) in enumerate(IMAGES[:2])]
    eng.set_images_ragged(tiles, slot0=0)
    _check(eng, [1, 0, 1], [5, 6, 2], "box", True, seed=21)          # chunks of 8 cross both boundaries
    _check(eng, [0, 1], [3, 3], "box_mask", False, seed=22)
    with eng.options(split=15):                                        # slot 2: a single-mask (1x-rate) embedding
        eng.set_images(torch.from_numpy(synth.make_image(42, *IMAGES[2][0])).cuda()[None], slot0=2)
    b, _, _, _ = _prompts("box", 4, 1)
    with pytest.raises(PrecisionError, match=r"slot 2"):
        eng.predict_multi([0, 2], [2, 2], b, None, None, None, True, False, [IMAGES[0][0], IMAGES[2][0]], [IMAGES[0][1], IMAGES[2][1]])
    _check(eng, [0, 2], [2, 2], "box", False, seed=23)                # single mask on it: fine
    eng.close()
