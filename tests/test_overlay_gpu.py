"""GPU: samrs_blend_labels / Engine.blend_labels against Pillow's Image.blend (tests/overlay_ref.py), bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from overlay_ref import overlay_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import samrs_amd
    sam = samrs_amd.sam_model_registry["vit_tiny"](max_prompts=4, max_points=1).to("cuda")
    return sam.engine


def _blend(eng, images, maps, lut, alpha):
    out = eng.blend_labels(torch.from_numpy(images).cuda(), torch.from_numpy(maps).cuda(), torch.from_numpy(lut).cuda(), alpha)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("alpha", [0.4, 0.0, 1.0, 1 / 3, 0.999])
def test_every_byte_pair_equals_pillow(eng, alpha):
    i = np.arange(256, dtype=np.uint8)
    image = np.ascontiguousarray(np.broadcast_to(i[:, None, None], (256, 256, 3)))        # image[i, j, :] = i
    seg = np.ascontiguousarray(np.broadcast_to(i[None, :], (256, 256)))                   # map[i, j] = j
    lut = np.ascontiguousarray(np.repeat(i[:, None], 3, axis=1))                          # lut[c] = (c, c, c)
    got = _blend(eng, image, seg, lut, alpha)
    want = overlay_ref(image, seg, lut, alpha)
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"alpha {alpha}: {len(bad)} bytes differ, first at (a, b, channel) = {bad[0].tolist()}"


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (5, 1), (33, 67), (517, 803)])
def test_tails_and_batch_equal_pillow(eng, hw):
    h, w = hw
    rng = np.random.default_rng(h * 1000 + w)
    images = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    maps = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    maps[:, 0, 0] = 255
    maps[1, h - 1, w - 1] = 255
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    got = _blend(eng, images, maps, lut, 0.4)
    for j in range(3):
        assert np.array_equal(got[j], overlay_ref(images[j], maps[j], lut, 0.4)), (hw, j)


def test_unaligned_views_take_the_scalar_path(eng):
    """Pointers that are not 16-byte aligned (a view one byte into a buffer) give the same bytes."""
    rng = np.random.default_rng(4)
    h, w = 19, 37
    image, seg = rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    ibuf = torch.zeros(h * w * 3 + 1, dtype=torch.uint8, device="cuda")
    mbuf = torch.zeros(h * w + 1, dtype=torch.uint8, device="cuda")
    obuf = torch.zeros(h * w * 3 + 1, dtype=torch.uint8, device="cuda")
    ibuf[1:].copy_(torch.from_numpy(image).reshape(-1))
    mbuf[1:].copy_(torch.from_numpy(seg).reshape(-1))
    eng.blend_labels(ibuf[1:].view(h, w, 3), mbuf[1:].view(h, w), torch.from_numpy(lut).cuda(), 0.4, out=obuf[1:])
    torch.cuda.synchronize()
    assert int(obuf[0]) == 0
    assert np.array_equal(obuf[1:].cpu().numpy().reshape(h, w, 3), overlay_ref(image, seg, lut, 0.4))


def test_bad_arguments_are_refused(eng):
    from samrs_amd import engine
    img = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device="cuda")
    seg = torch.zeros(1, 4, 4, dtype=torch.uint8, device="cuda")
    lut = torch.zeros(256, 3, dtype=torch.uint8, device="cuda")
    out = torch.full_like(img, 7)
    args = (eng.handle, img.data_ptr(), seg.data_ptr(), lut.data_ptr())
    for alpha in (-0.01, 1.01, float("nan")):
        assert eng.lib.samrs_blend_labels(*args, alpha, out.data_ptr(), 1, 4, 4, None) == engine.ERR_BAD_ARG, alpha
    for n, h, w in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4), (1, 4, -4)):
        assert eng.lib.samrs_blend_labels(*args, 0.4, out.data_ptr(), n, h, w, None) == engine.ERR_BAD_ARG, (n, h, w)
    assert eng.lib.samrs_blend_labels(*args, 0.4, img.data_ptr(), 1, 4, 4, None) == engine.ERR_BAD_ARG      # out aliases images
    torch.cuda.synchronize()
    assert bool((out == 7).all())
    with pytest.raises(AssertionError):
        eng.blend_labels(img, seg, lut, 1.5)
