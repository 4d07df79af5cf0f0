"""GPU: the five grow-on-demand scratch buffers an engine keeps between calls (engine_state.h DeviceScratch / scratch_reserve), each
through an entry point that uses it: samrs_rle_encode interleaved with samrs_rle_encode_placed (they share one), samrs_clean_masks,
samrs_mask_boxes, samrs_mask_polygons, samrs_png_encode_labels.  On ONE engine each takes three calls in order:

    small        2 masks of 16 x 16: the first allocation;
    large        34 masks of 48 x 64: the scratch grows, and the 32-mask chunk loops (RLE, REGION_CHUNK) take two passes;
    small again  2 masks of 16 x 16: the oversized scratch is reused.

Every result is compared for exact equality with the host reference the feature's own GPU test uses (samrs_amd/rle.py,
tests/region_ref.py, tests/box_ref.py, tests/polygon_ref.py, libsamrs_io.so's PNG writer).  The masks are random (fixed seed, density
0.5) plus one all-zero and one all-one mask per stack; in the large stack those two sit at indices 31 and 32, either side of the chunk
boundary.  Nothing here looks at a pointer or a size: what is checked is that a call's answer does not depend on the calls before it."""
import os
import sys

import numpy as np
import pytest
import torch

from samrs_amd import rle, tile_io

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import box_ref  # noqa: E402
import polygon_ref  # noqa: E402
import region_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import samrs_amd
    sam = samrs_amd.sam_model_registry["vit_tiny"](max_images=1, max_prompts=4).to("cuda")
    return sam.engine


@pytest.fixture(scope="module")
def stacks():
    """the three calls' masks, in call order: uint8 [2, 16, 16], [34, 48, 64], [2, 16, 16]"""
    rng = np.random.default_rng(20)
    small = (rng.random((2, 16, 16)) < 0.5).astype(np.uint8)
    small[1] = 0
    large = (rng.random((34, 48, 64)) < 0.5).astype(np.uint8)
    large[31] = 0
    large[32] = 1
    again = (rng.random((2, 16, 16)) < 0.5).astype(np.uint8)
    again[0] = 1
    for m in (small, large, again):
        m.setflags(write=False)
    return small, large, again


def _dev(masks):
    return torch.from_numpy(np.array(masks)).cuda()


def _strings(out, tab):
    o = out.cpu().numpy()
    return [o[int(off):int(off) + int(n)].tobytes().decode("ascii") for off, n, _ in tab.cpu().numpy()]


def test_rle_and_placed_rle_share_one_scratch(eng, stacks):
    x0, y0 = 3, 5
    for k, masks in enumerate(stacks):
        n, h, w = masks.shape
        H, W = h + 11, w + 6
        pasted = np.zeros((n, H, W), np.uint8)
        pasted[:, y0:y0 + h, x0:x0 + w] = masks
        for placed, frames in ((False, masks), (True, pasted)):
            out = torch.zeros(n * (2 * H * W + 64) + 64, dtype=torch.uint8, device="cuda")
            cur = torch.zeros(1, dtype=torch.int64, device="cuda")
            tab = torch.zeros(n, 3, dtype=torch.int64, device="cuda")
            if placed:
                eng.rle_encode_placed(_dev(masks), (x0, y0, w, h), (H, W), out, cur, tab)
            else:
                eng.rle_encode(_dev(masks), out, cur, tab)
            torch.cuda.synchronize()
            want = [rle.encode(f)["counts"] for f in frames]
            assert _strings(out, tab) == want, f"call {k}, placed={placed}"
            assert tab[:, 2].cpu().tolist() == [len(rle.mask_to_counts(f)) for f in frames], f"call {k}, placed={placed}: n_counts"


def test_clean_masks(eng, stacks):
    for k, masks in enumerate(stacks):
        d = _dev(masks)
        _, areas, changed = eng.clean_masks(d, 4, "both")
        torch.cuda.synchronize()
        want, wa, wc = region_ref.clean_batch(masks, 4, "both")
        assert np.array_equal(d.cpu().numpy(), want), f"call {k}: masks"
        assert np.array_equal(areas.cpu().numpy(), wa) and np.array_equal(changed.cpu().numpy(), wc), f"call {k}: areas / changed"


def test_mask_boxes(eng, stacks):
    for k, masks in enumerate(stacks):
        got = eng.mask_boxes(_dev(masks), (7, 9))
        torch.cuda.synchronize()
        for name, g, w in zip(("hbox", "rbox", "record"), got, box_ref.mask_boxes(masks, 7, 9)):
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f"call {k}: {name}"


def test_mask_polygons(eng, stacks):
    for k, masks in enumerate(stacks):
        v, r, c, t = (x.cpu().numpy() for x in eng.mask_polygons(_dev(masks)))
        want_v, want_r, want_c, want_t = polygon_ref.mask_polygons(masks)
        assert t.tolist() == want_t.tolist(), f"call {k}: table"
        assert tuple(c.tolist()) == tuple(want_c), f"call {k}: cursor"
        assert np.array_equal(v[:want_c[0]], want_v) and np.array_equal(r[:want_c[1]], want_r), f"call {k}: vertices / rings"


def test_png_encode_labels(eng, stacks, tmp_path):
    lut = tile_io.class_lut(np.random.default_rng(3).integers(0, 256, (2, 3), dtype=np.uint8))
    g, c = str(tmp_path / "g.png"), str(tmp_path / "c.png")
    for k, maps in enumerate(stacks):                        # the masks as class maps of labels 0 and 1
        n, h, w = maps.shape
        out = torch.zeros(n * 2 * (h * w * 6 + h * 2 + 8192) + 4096, dtype=torch.uint8, device="cuda")
        cur = torch.zeros(1, dtype=torch.int64, device="cuda")
        tab = torch.zeros(n, 2, 2, dtype=torch.int64, device="cuda")
        eng.png_encode(_dev(maps), torch.from_numpy(lut).cuda(), out, cur, tab)
        torch.cuda.synchronize()
        o, tab = out.cpu().numpy(), tab.cpu().numpy()
        for j in range(n):
            tile_io.write_label_pair(g, c, np.ascontiguousarray(maps[j]), lut)
            for kind, path in enumerate((g, c)):
                with open(path, "rb") as f:
                    want = f.read()
                off, size = int(tab[j, kind, 0]), int(tab[j, kind, 1])
                assert size == len(want) and bytes(o[off:off + size]) == want, f"call {k}, map {j}, {'gray colour'.split()[kind]}"
