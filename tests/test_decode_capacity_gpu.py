"""GPU: the decoder's chain capacity (engine option "decode_prompts") apart from max_prompts.  A chain longer than max_prompts --
the prompts of several images in ONE pass of samrs_predict_multi -- gives what the chunked call and the per-image calls give, bit
for bit: masks, IoU predictions, low-res logits.  Growing the workspaces, the refusals, ragged and empty segments, and the
pipelines' batch_decode="auto"."""
import numpy as np
import pytest
import torch

import test_predict_multi_gpu as tpm
from samrs_amd import synth

pytestmark = pytest.mark.gpu

# (input size, original size) per slot: native, shown smaller, ragged -- the post-processing runs per image segment with these
IMAGES = tpm.IMAGES
MAX_IMAGES, MAX_PROMPTS, CHAIN = 3, 2, 6
_ENGINES = {}


def _new_engine(precision="f16", fused=True, options=None):
    import samrs_amd
    opts = dict(options or {})
    if not fused:
        opts["decoder_fusion"] = 0
    sam = samrs_amd.sam_model_registry["vit_tiny"](precision=precision, max_images=MAX_IMAGES, max_prompts=MAX_PROMPTS, max_points=4,
                                                   options=opts or None).to("cuda")
    tiles = [torch.from_numpy(synth.make_image(60 + i, *ins)).cuda() for i, (ins, _) in enumerate(IMAGES)]
    sam.engine.set_images_ragged(tiles, slot0=0)
    return sam.engine


def _engine(precision, fused):
    key = (precision, fused)
    if key not in _ENGINES:
        _ENGINES[key] = _new_engine(precision, fused)
    return _ENGINES[key]


def _call(eng, slots, counts, per, multimask):
    sizes = [IMAGES[s] for s in slots]
    args = [tpm._cat([p[j] for p in per]) for j in range(4)]
    return eng.predict_multi(slots, counts, *args, multimask, False, [s[0] for s in sizes], [s[1] for s in sizes])


def _same_outputs(a, b):
    for x, y in zip(a, b):                     # masks, iou, low: per-image lists
        assert len(x) == len(y)
        for u, v in zip(x, y):
            tpm._same(u, v)


def _chain_equals_chunks(eng, slots, counts, kind, multimask, seed):
    """One chain of sum(counts) prompts == the same call in chunks of <= max_prompts == one predict per image."""
    per = [tpm._prompts(kind, n, seed + 7 * i, IMAGES[s][0]) for i, (s, n) in enumerate(zip(slots, counts))]
    eng.set_option("decode_prompts", MAX_PROMPTS)                  # the default capacity: chunks of <= 2
    chunked = _call(eng, slots, counts, per, multimask)
    single = [eng.predict(s, *per[i], multimask, False, *IMAGES[s]) if n else None for i, (s, n) in enumerate(zip(slots, counts))]
    eng.set_option("decode_prompts", CHAIN)
    assert eng.get_option("decode_prompts") == CHAIN and sum(counts) > MAX_PROMPTS
    chain = _call(eng, slots, counts, per, multimask)
    _same_outputs(chain, chunked)
    c = 3 if multimask else 1
    for i, (s, n) in enumerate(zip(slots, counts)):
        oh, ow = IMAGES[s][1]
        assert tuple(chain[0][i].shape) == (n, c, oh, ow) and tuple(chain[1][i].shape) == (n, c)
        assert tuple(chain[2][i].shape) == (n, c, 256, 256)
        if n:
            for j in range(3):
                tpm._same(chain[j][i], single[i][j])
    torch.cuda.synchronize()


KINDS = ["box", "pt3", "box_mask"]       # box_mask: the non-shared layer 0 (DENSE, make_keys through the slot table)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_segment"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("multimask", [False, True])
@pytest.mark.parametrize("precision", ["f16", "bf16"])
def test_chain_equals_chunks(precision, multimask, kind, fused):
    """max_images = 3, max_prompts = 2, prompts 2 + 1 + 2: decode_prompts = 6 runs them as one chain of 5."""
    _chain_equals_chunks(_engine(precision, fused), [0, 1, 2], [2, 1, 2], kind, multimask,
                         seed=3 * KINDS.index(kind) + int(multimask))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_segment"])
@pytest.mark.parametrize("counts", [[0, 2, 1], [2, 0, 0], [2, 2, 2]])
def test_ragged_and_empty_segments(counts, fused):
    """An image without prompts is no segment of the chain (nothing is launched for it; its outputs are empty); [2, 2, 2] fills the
    capacity to the last prompt."""
    eng = _engine("f16", fused)
    if sum(counts) > MAX_PROMPTS:
        _chain_equals_chunks(eng, [0, 1, 2], counts, "box", True, seed=31)
        _chain_equals_chunks(eng, [2, 0, 1], counts, "box_mask", False, seed=32)
    else:                                                             # a chain no longer than max_prompts: still through the capacity
        per = [tpm._prompts("box", n, 33 + i, IMAGES[s][0]) for i, (s, n) in enumerate(zip([0, 1, 2], counts))]
        eng.set_option("decode_prompts", CHAIN)
        got = _call(eng, [0, 1, 2], counts, per, True)
        m0, q0, l0 = eng.predict(0, *per[0], True, False, *IMAGES[0])
        tpm._same(got[0][0], m0), tpm._same(got[1][0], q0), tpm._same(got[2][0], l0)
        assert got[0][1].shape[0] == 0 and got[0][2].shape[0] == 0 and got[2][1].shape[0] == 0


def test_growth_and_refusals():
    from samrs_amd.engine import ERR_BAD_ARG
    eng = _new_engine()
    slots, counts = [0, 1, 2], [2, 1, 2]
    per = [tpm._prompts("box_mask", n, 40 + i, IMAGES[s][0]) for i, (s, n) in enumerate(zip(slots, counts))]
    assert eng.get_option("decode_prompts") == MAX_PROMPTS            # the default: nothing changes for existing callers
    before = _call(eng, slots, counts, per, True)                     # a predict has run (chunks of 2; SLOT_OF and DENSE exist)
    kb0 = eng.get_option("decode_kbytes")
    eng.set_option("decode_prompts", CHAIN)
    kb1 = eng.get_option("decode_kbytes")
    assert kb0 > 0 and kb1 == pytest.approx(kb0 * CHAIN / MAX_PROMPTS, abs=2)      # every buffer is linear in the capacity
    eng.set_option("decode_prompts", CHAIN)                           # the same value again: nothing new
    assert eng.get_option("decode_kbytes") == kb1
    grown = _call(eng, slots, counts, per, True)
    _same_outputs(grown, before)
    fresh_eng = _new_engine(options={"decode_prompts": CHAIN})        # created at the larger capacity
    assert fresh_eng.get_option("decode_prompts") == CHAIN
    _same_outputs(_call(fresh_eng, slots, counts, per, True), grown)
    assert fresh_eng.get_option("decode_kbytes") == kb1
    fresh_eng.close()
    # the range: [max_prompts, max_images x max_prompts]
    for bad in (MAX_PROMPTS - 1, 0, -1, MAX_IMAGES * MAX_PROMPTS + 1, 1 << 20):
        rc = eng.lib.samrs_set_option(eng.handle, b"decode_prompts", bad)
        msg = eng.lib.samrs_last_error(eng.handle).decode()
        assert rc == ERR_BAD_ARG and f"[{MAX_PROMPTS}, {MAX_IMAGES * MAX_PROMPTS}]" in msg, (bad, rc, msg)
        assert eng.get_option("decode_prompts") == CHAIN and eng.get_option("decode_kbytes") == kb1
    # never shrinks: a lower value shortens the chains and keeps the memory
    eng.set_option("decode_prompts", MAX_PROMPTS)
    assert eng.get_option("decode_prompts") == MAX_PROMPTS and eng.get_option("decode_kbytes") == kb1
    _same_outputs(_call(eng, slots, counts, per, True), grown)
    eng.close()


def test_single_image_predict_keeps_its_contract():
    """samrs_predict is untouched by the capacity: n = max_prompts + 1 on one image does what it did before this option existed.
    That is NOT a refusal: samrs_predict never refused a long call, it runs it in passes of max_prompts
    (test_pipeline_gpu.py::test_predict_batches_beyond_max_prompts pins that), with or without a raised capacity."""
    eng = _engine("f16", True)
    b, pc, pl, mi = tpm._prompts("box", MAX_PROMPTS + 1, 50)
    outs = []
    for cap in (MAX_PROMPTS, CHAIN):
        eng.set_option("decode_prompts", cap)
        outs.append(eng.predict(0, b, pc, pl, mi, True, False, *IMAGES[0]))
    parts = [eng.predict(0, b[s:e], None, None, None, True, False, *IMAGES[0]) for s, e in [(0, MAX_PROMPTS), (MAX_PROMPTS, MAX_PROMPTS + 1)]]
    for j in range(3):
        tpm._same(outs[0][j], outs[1][j])
        tpm._same(outs[0][j], torch.cat([p[j] for p in parts]))


def test_tile_pipeline_auto_equals_per_tile():
    """TilePipeline(batch=2), 3 boxes on each of 4 tiles: "auto" resolves to on, raises the engine's decode_prompts to 6 and decodes
    each batch as one chain; class maps, areas and class statistics equal the per-tile run byte for byte."""
    import samrs_amd
    from samrs_amd import driver
    sam = samrs_amd.sam_model_registry["vit_tiny"](precision="f16", max_images=4, max_prompts=3, max_points=1).to("cuda")
    items = []
    for i in range(4):
        boxes, labels = synth.make_boxes(70 + i, 3, 1024, 1024)
        items.append(driver.WorkItem(f"img{i}", synth.make_image(70 + i, 1024, 1024), boxes, labels))

    def collect(mode):
        pipe = driver.TilePipeline(sam, 18, batch=2, box_batch=3, max_boxes=3, batch_decode=mode)
        got = {}

        def sink(results, release):
            for r in results:
                got[r.key] = (r.seg_mask.copy(), r.areas.copy())
            release()
        assert pipe.run(driver.batched(items, 2), sink) == len(items)
        return pipe, got, pipe.class_pixels.cpu(), pipe.class_instances.cpu()

    p0, ref, cp0, ci0 = collect(False)
    assert not p0.batch_decode_on and sam.engine.get_option("decode_prompts") == 3
    p1, got, cp1, ci1 = collect("auto")
    assert p1.batch_decode_on and sam.engine.get_option("decode_prompts") == 6, p1.batch_decode_reason
    assert sorted(ref) == sorted(got) and len(got) == 4
    for k in ref:
        assert ref[k][0].tobytes() == got[k][0].tobytes() and ref[k][1].tobytes() == got[k][1].tobytes(), k
        assert (got[k][0] != 255).any()
    assert np.array_equal(cp0.numpy(), cp1.numpy()) and np.array_equal(ci0.numpy(), ci1.numpy())
    assert int(ci1.sum()) > 0
