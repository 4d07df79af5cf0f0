"""GPU: Sam.forward / Sam.__call__ (modeling/sam.py:53-131) -- a list of images, each with its own prompts -- against the
SamPredictor.set_torch_image / predict_torch loop, byte for byte (the loop is what the golden fixtures pin)."""
import numpy as np
import pytest
import torch

from samrs_amd import synth

pytestmark = pytest.mark.gpu


def _sam(max_images=3, name="vit_tiny"):
    import samrs_amd
    return samrs_amd.sam_model_registry[name](precision="f16", max_images=max_images, max_prompts=16, max_points=4).to("cuda")


def _record(i, hw, orig, kind, n):
    """One batched_input record: a float 3xHxW image of integer values and `kind` prompts in its input frame."""
    h, w = hw
    rng = np.random.default_rng(100 + i)
    r = {"image": torch.from_numpy(synth.make_image(60 + i, h, w)).permute(2, 0, 1).float().cuda(), "original_size": orig}
    if "box" in kind:
        r["boxes"] = torch.from_numpy(synth.make_boxes(60 + i, n, h, w)[0]).cuda()
    if "pt" in kind:
        k = 2 if "pt2" in kind else 1
        r["point_coords"] = torch.from_numpy(np.stack([rng.uniform(0, w, (n, k)), rng.uniform(0, h, (n, k))], -1)
                                             .astype(np.float32)).cuda()
        r["point_labels"] = torch.from_numpy(rng.integers(0, 2, (n, k)).astype(np.int32)).cuda()
    if "mask" in kind:
        r["mask_inputs"] = torch.from_numpy(rng.normal(0, 4, (n, 1, 256, 256)).astype(np.float32)).cuda()
    return r


def _loop(sam, batch, multimask):
    import samrs_amd
    pred = samrs_amd.SamPredictor(sam)
    out = []
    for r in batch:
        pred.set_torch_image(r["image"][None], r["original_size"])
        m, q, l = pred.predict_torch(r.get("point_coords"), r.get("point_labels"), r.get("boxes"), r.get("mask_inputs"),
                                     multimask_output=multimask)
        out.append((m.cpu(), q.cpu(), l.cpu()))
    return out


def _assert_same(got, want):
    assert len(got) == len(want)
    for g, (m, q, l) in zip(got, want):
        assert set(g) == {"masks", "iou_predictions", "low_res_logits"}
        assert g["masks"].dtype == torch.bool and torch.equal(g["masks"].cpu(), m)
        assert torch.equal(g["iou_predictions"].cpu().view(torch.int32), q.view(torch.int32))
        assert torch.equal(g["low_res_logits"].cpu().view(torch.int32), l.view(torch.int32))


BATCH = [((1024, 1024), (1024, 1024), "box", 4), ((1024, 1024), (800, 800), "pt2", 3), ((600, 1024), (600, 1024), "mask", 2),
         ((1024, 1024), (2048, 2048), "box", 5), ((1024, 768), (1024, 768), "box_pt1", 2), ((1024, 1024), (1024, 1024), "box_mask", 1)]


@pytest.mark.parametrize("multimask", [False, True])
def test_forward_equals_predictor_loop(multimask):
    sam = _sam(max_images=7)
    batch = [_record(i, *b) for i, b in enumerate(BATCH)]
    got = sam(batch, multimask)
    _assert_same(got, _loop(sam, batch, multimask))
    c = 3 if multimask else 1
    for g, (_, orig, _, n) in zip(got, BATCH):
        assert tuple(g["masks"].shape) == (n, c, *orig)


def test_batch_larger_than_the_slots():
    """max_images = 3: two free slots, six images -> three encoder chunks; mixed prompt kinds inside each chunk."""
    sam = _sam(max_images=3)
    batch = [_record(i, *b) for i, b in enumerate(BATCH)]
    _assert_same(sam.forward(batch, True), _loop(sam, batch, True))


def test_predictor_unchanged_by_forward():
    import samrs_amd
    sam = _sam(max_images=3)
    pred = samrs_amd.SamPredictor(sam)
    img = synth.make_image(7)
    pred.set_image(img)
    bx = torch.from_numpy(synth.make_boxes(7, 6)[0]).cuda()
    before = [t.cpu() for t in pred.predict_torch(None, None, bx, None, multimask_output=True)]
    sam([_record(i, *b) for i, b in enumerate(BATCH)], True)
    after = [t.cpu() for t in pred.predict_torch(None, None, bx, None, multimask_output=True)]
    for a, b in zip(before, after):
        assert torch.equal(a.view(torch.uint8) if a.dtype == torch.bool else a.view(torch.int32),
                           b.view(torch.uint8) if b.dtype == torch.bool else b.view(torch.int32))
    assert sam.engine.get_slot_info(0)["is_set"] == 1


def test_forward_needs_a_free_slot_and_valid_images():
    sam = _sam(max_images=1)
    with pytest.raises(RuntimeError, match="max_images"):
        sam([_record(0, *BATCH[0])], False)
    sam = _sam(max_images=2)
    bad = _record(0, *BATCH[0])
    bad["image"] = bad["image"] + 0.5
    with pytest.raises(AssertionError, match="0..255"):
        sam([bad], False)
    small = _record(0, (512, 512), (512, 512), "box", 2)
    with pytest.raises(AssertionError, match="long side"):
        sam([small], False)
