"""GPU: scene mode.  The compositing kernels alone (samrs_scene_claim / samrs_scene_resolve, samrs_rle_encode_placed) against
the numpy restatement tests/scene_ref.py, then ScenePipeline end to end against a manual composition through SamPredictor,
against TilePipeline on scenes no larger than the window, with the small-region clean-up, and through the generation CLI.
Integer work on both sides of every comparison: all of them are exact."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from samrs_amd import rle, synth, tile_io

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import region_ref  # noqa: E402
import scene_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N_CLASSES = 18


@pytest.fixture(scope="module")
def sam():
    import samrs_amd
    return samrs_amd.sam_model_registry["vit_tiny"](max_images=8, max_prompts=64, precision="f16").to("cuda")


@pytest.fixture(scope="module")
def eng(sam):
    return sam.engine


# ---- 1. claim + resolve alone ---------------------------------------------------------------------------------------------------

def _masks(rng, n, h, w, density):
    m = (rng.random((n, h, w)) < density).astype(np.uint8)
    m[m != 0] = rng.integers(1, 256, int(m.sum()), dtype=np.uint8)              # non-zero = set, not only 1
    if n >= 3:
        m[0] = 0                                                                 # an all-zero mask
        m[1] = 255                                                               # an all-ones mask
    return m


def _new_order(H, W):
    return torch.full((H, W), -1, dtype=torch.int32, device="cuda")


def _claim(eng, masks, ranks, win, order, labels_by_rank, stats=True):
    n = len(masks)
    lab = torch.from_numpy(np.asarray(labels_by_rank, np.int32)[np.asarray(ranks)]).cuda()
    pix = torch.zeros(N_CLASSES, dtype=torch.int64, device="cuda") if stats else None
    ins = torch.zeros(N_CLASSES, dtype=torch.int64, device="cuda") if stats else None
    areas = eng.scene_claim(torch.from_numpy(masks).cuda(), torch.from_numpy(np.asarray(ranks, np.int32)).cuda(), win, order,
                            lab if stats else None, pix, ins)
    torch.cuda.synchronize()
    assert areas.numel() == n
    return areas.cpu().numpy(), (pix.cpu().numpy(), ins.cpu().numpy()) if stats else None


# (w, h, x0, y0, H, W)
GEOMETRIES = {
    "odd_width_unaligned_origin": (37, 53, 5, 7, 64, 96),           # bytewise mask path
    "sixteen_byte_path": (48, 64, 32, 16, 89, 93),                   # 16-byte mask loads; map rows of mixed alignment
    "flush_bottom_right": (32, 20, 38, 30, 50, 70),
    "window_is_the_canvas": (64, 48, 0, 0, 48, 64),
}


@pytest.mark.parametrize("density", [0.3, 0.7])
@pytest.mark.parametrize("n", [1, 3, 70])                            # 70: more than one counter chunk of 64
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_claim_and_resolve_equal_the_host_composition(eng, geometry, n, density):
    w, h, x0, y0, H, W = GEOMETRIES[geometry]
    rng = np.random.default_rng(1000 * list(GEOMETRIES).index(geometry) + 10 * n + int(density * 10))
    masks = _masks(rng, n, h, w, density)
    ranks = rng.permutation(n).astype(np.int32)                      # any order: the rule is "highest rank", not "last mask"
    labels_by_rank = rng.integers(0, N_CLASSES, n).astype(np.int32)
    order = _new_order(H, W)
    areas, (pix, ins) = _claim(eng, masks, ranks, (x0, y0, w, h), order, labels_by_rank)
    seg = eng.scene_resolve(order, torch.from_numpy(labels_by_rank).cuda()).cpu().numpy()
    want_seg, want_areas = scene_ref.composite([(masks, ranks, (x0, y0, w, h))], labels_by_rank, H, W)
    want_order = np.full((H, W), -1, np.int32)
    for j in np.argsort(ranks):
        want_order[y0:y0 + h, x0:x0 + w][masks[j] != 0] = ranks[j]
    assert np.array_equal(order.cpu().numpy(), want_order)
    assert np.array_equal(seg, want_seg)
    assert np.array_equal(areas, want_areas[ranks])
    # areas and class arrays: exactly samrs_paint's on the same masks
    p_pix = torch.zeros(N_CLASSES, dtype=torch.int64, device="cuda")
    p_ins = torch.zeros(N_CLASSES, dtype=torch.int64, device="cuda")
    p_seg = torch.full((h, w), 255, dtype=torch.uint8, device="cuda")
    p_areas = eng.paint(torch.from_numpy(masks).cuda(), torch.from_numpy(labels_by_rank[ranks]).cuda(), p_seg, p_pix, p_ins)
    assert np.array_equal(areas, p_areas.cpu().numpy())
    assert np.array_equal(pix, p_pix.cpu().numpy()) and np.array_equal(ins, p_ins.cpu().numpy())
    assert np.array_equal((pix, ins), scene_ref.class_stats(areas, labels_by_rank[ranks], N_CLASSES))


def test_two_overlapping_windows_in_either_call_order(eng):
    H, W = 80, 120
    rng = np.random.default_rng(5)
    win_a, win_b = (8, 4, 64, 48), (40, 20, 48, 60)                   # they share 32 x 32 pixels
    ranks_a, ranks_b = np.array([0, 2, 5], np.int32), np.array([1, 3, 4], np.int32)
    masks_a = (rng.random((3, 48, 64)) < 0.5).astype(np.uint8)
    masks_b = (rng.random((3, 60, 48)) < 0.5).astype(np.uint8)
    labels = np.array([3, 7, 1, 0, 11, 5], np.int32)
    want_seg, want_areas = scene_ref.composite([(masks_a, ranks_a, win_a), (masks_b, ranks_b, win_b)], labels, H, W)
    segs = []
    for first in ("a", "b"):
        order = _new_order(H, W)
        calls = [(masks_a, ranks_a, win_a), (masks_b, ranks_b, win_b)]
        got = np.zeros(6, np.int64)
        for masks, ranks, win in (calls if first == "a" else calls[::-1]):
            got[ranks] = _claim(eng, masks, ranks, win, order, labels)[0]
        segs.append(eng.scene_resolve(order, torch.from_numpy(labels).cuda()).cpu().numpy())
        assert np.array_equal(got, want_areas)
    assert np.array_equal(segs[0], segs[1]) and np.array_equal(segs[0], want_seg)
    # the highest rank wins wherever both windows have a mask set
    both = scene_ref.paste(masks_a[2], 8, 4, H, W) & scene_ref.paste(masks_b[2], 40, 20, H, W)           # ranks 5 and 4
    assert both.any() and np.all(segs[0][both] == labels[5])


def test_claim_without_areas_or_labels_and_with_no_masks(eng):
    rng = np.random.default_rng(8)
    masks = (rng.random((2, 16, 32)) < 0.5).astype(np.uint8)
    order = _new_order(40, 40)
    _claim(eng, masks, [1, 0], (3, 5, 32, 16), order, [4, 9], stats=False)
    seg = eng.scene_resolve(order, torch.tensor([4, 9], dtype=torch.int32, device="cuda")).cpu().numpy()
    assert np.array_equal(seg, scene_ref.composite([(masks, [1, 0], (3, 5, 32, 16))], [4, 9], 40, 40)[0])
    empty = _new_order(12, 20)
    eng.scene_claim(torch.zeros(0, 12, 20, dtype=torch.uint8, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                    (0, 0, 20, 12), empty)
    seg = eng.scene_resolve(empty, torch.zeros(0, dtype=torch.int32, device="cuda")).cpu().numpy()
    assert np.all(seg == 255)


@pytest.mark.parametrize("win", [(60, 0, 16, 8), (0, 44, 16, 8), (-1, 0, 16, 8), (0, -1, 16, 8)])
def test_window_outside_the_canvas_is_refused_and_nothing_is_written(eng, win):
    from samrs_amd.engine import EngineError
    order = _new_order(48, 64)
    areas = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    masks = torch.ones(2, 8, 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(EngineError, match="not inside"):
        eng.scene_claim(masks, torch.tensor([0, 1], dtype=torch.int32, device="cuda"), win, order, areas_out=areas)
    out = torch.full((4096,), 0xAB, dtype=torch.uint8, device="cuda")
    cur = torch.zeros(1, dtype=torch.int64, device="cuda")
    tab = torch.full((2, 3), -7, dtype=torch.int64, device="cuda")
    with pytest.raises(EngineError, match="not inside"):
        eng.rle_encode_placed(masks, win, (48, 64), out, cur, tab)
    torch.cuda.synchronize()
    assert bool((order == -1).all()) and bool((areas == -7).all())
    assert bool((out == 0xAB).all()) and int(cur.item()) == 0 and bool((tab == -7).all())


# ---- 2. rle_encode_placed alone -------------------------------------------------------------------------------------------------

def _placed(eng, masks, win, size, out=None, cur=None, cap=1 << 20):
    n = len(masks)
    if out is None:
        out = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
    if cur is None:
        cur = torch.zeros(1, dtype=torch.int64, device="cuda")
    tab = torch.zeros(n, 3, dtype=torch.int64, device="cuda")
    eng.rle_encode_placed(torch.from_numpy(np.ascontiguousarray(masks)).cuda(), win, size, out, cur, tab)
    torch.cuda.synchronize()
    return out, cur, tab.cpu().numpy()


def _strings(out, tab):
    o = out.cpu().numpy()
    return [o[int(off):int(off) + int(n)].tobytes().decode("ascii") for off, n, _ in tab]


def _check_placed(eng, masks, win, size):
    x0, y0, w, h = win
    H, W = size
    out, cur, tab = _placed(eng, masks, win, size)
    want = [scene_ref.scene_rle(m, x0, y0, H, W) for m in masks]
    assert _strings(out, tab) == [r["counts"] for r in want]
    n_counts = [len(rle.mask_to_counts(scene_ref.paste(m, x0, y0, H, W))) for m in masks]
    assert tab[:, 2].tolist() == n_counts
    assert np.all(tab[:, 0] % 16 == 0)
    for r, m in zip(want, masks):                                    # and the reference strings decode to the pasted masks
        assert np.array_equal(rle.decode(r), scene_ref.paste(m, x0, y0, H, W))
    return tab


@pytest.mark.parametrize("x0", [0, "last"])
@pytest.mark.parametrize("y0", [0, 7, 33])
@pytest.mark.parametrize("H", [45, 130])                             # not multiples of 32
def test_placed_rle_equals_the_rle_of_the_pasted_mask(eng, H, y0, x0):
    W, w, h = 40, 9, 10
    rng = np.random.default_rng(H + y0)
    masks = np.stack([(rng.random((h, w)) < 0.5).astype(np.uint8), np.ones((h, w), np.uint8), np.zeros((h, w), np.uint8),
                      (rng.random((h, w)) < 0.9).astype(np.uint8) * 200])
    masks[3][:, -1] = 1                                              # the window's last column set to its bottom
    _check_placed(eng, masks, (W - w if x0 == "last" else 0, y0, w, h), (H, W))


def test_placed_rle_over_several_blocks_of_rows_and_columns(eng):
    rng = np.random.default_rng(3)
    masks = (rng.random((2, 100, 300)) < 0.5).astype(np.uint8)      # 300 columns: three column chunks; canvas of two row blocks
    _check_placed(eng, masks, (3, 7, 300, 100), (130, 310))
    masks = (rng.random((2, 130, 131)) < 0.5).astype(np.uint8)      # full height, odd width, x0 > 0, touching the right edge
    _check_placed(eng, masks, (179, 0, 131, 130), (130, 310))
    masks = (rng.random((33, 20, 24)) < 0.3).astype(np.uint8)       # more masks than one pass holds
    _check_placed(eng, masks, (5, 9, 24, 20), (45, 64))


def test_runs_join_across_columns_only_at_full_height(eng):
    H, W, w, x0 = 45, 40, 5, 11
    full = np.ones((1, H, w), np.uint8)
    tab = _check_placed(eng, full, (x0, 0, w, H), (H, W))
    assert tab[0, 2] == 3                                            # zeros, one run of w H ones, zeros
    assert rle.string_to_counts(_strings(*_placed(eng, full, (x0, 0, w, H), (H, W))[::2])[0]) == [x0 * H, w * H, (W - x0 - w) * H]
    for y0, h in ((0, H - 1), (1, H - 1), (3, 20)):                  # the same set columns, not full height: one run per column
        tab = _check_placed(eng, np.ones((1, h, w), np.uint8), (x0, y0, w, h), (H, W))
        assert tab[0, 2] == 2 * w + 1
    tab = _check_placed(eng, np.ones((1, H, w), np.uint8), (W - w, 0, w, H), (H, W))       # up to the canvas's last pixel
    assert tab[0, 2] == 2


def test_empty_mask_and_full_canvas(eng):
    H, W = 45, 52
    out, _, tab = _placed(eng, np.zeros((1, 10, 9), np.uint8), (4, 7, 9, 10), (H, W))
    assert tab[0, 2] == 1 and rle.string_to_counts(_strings(out, tab)[0]) == [H * W]
    out, _, tab = _placed(eng, np.ones((1, H, W), np.uint8), (0, 0, W, H), (H, W))
    assert tab[0, 2] == 2 and rle.string_to_counts(_strings(out, tab)[0]) == [0, H * W]
    _check_placed(eng, np.ones((1, H, W), np.uint8), (0, 0, W, H), (H, W))


def test_placed_rle_of_the_whole_frame_equals_rle_encode(eng):
    rng = np.random.default_rng(21)
    masks = (rng.random((3, 130, 72)) < 0.4).astype(np.uint8)
    out, _, tab = _placed(eng, masks, (0, 0, 72, 130), (130, 72))
    out2 = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    cur2 = torch.zeros(1, dtype=torch.int64, device="cuda")
    tab2 = torch.zeros(3, 3, dtype=torch.int64, device="cuda")
    eng.rle_encode(torch.from_numpy(masks).cuda(), out2, cur2, tab2)
    assert np.array_equal(tab, tab2.cpu().numpy()) and _strings(out, tab) == _strings(out2, tab2.cpu().numpy())


def test_two_placed_calls_append_behind_one_cursor(eng):
    rng = np.random.default_rng(9)
    a, b = (rng.random((2, 10, 9)) < 0.5).astype(np.uint8), (rng.random((1, 30, 17)) < 0.5).astype(np.uint8)
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    cur = torch.full((1,), 37, dtype=torch.int64, device="cuda")
    _, _, ta = _placed(eng, a, (3, 7, 9, 10), (45, 40), out=out, cur=cur)
    end_a = int(cur.item())
    _, _, tb = _placed(eng, b, (20, 1, 17, 30), (45, 40), out=out, cur=cur)
    assert ta[0, 0] == 48 and tb[0, 0] == end_a and end_a == ta[1, 0] + (ta[1, 1] + 15) // 16 * 16
    assert int(cur.item()) == tb[0, 0] + (tb[0, 1] + 15) // 16 * 16
    assert _strings(out, ta) == [scene_ref.scene_rle(m, 3, 7, 45, 40)["counts"] for m in a]
    assert _strings(out, tb) == [scene_ref.scene_rle(m, 20, 1, 45, 40)["counts"] for m in b]


def test_placed_rle_too_small_a_buffer_reports_the_size(eng):
    rng = np.random.default_rng(13)
    one = np.zeros((60, 64), np.uint8)
    one[17, 40] = 1
    masks = np.stack([np.zeros((60, 64), np.uint8), (rng.random((60, 64)) < 0.5).astype(np.uint8), one])
    want = [scene_ref.scene_rle(m, 5, 9, 130, 90)["counts"] for m in masks]
    assert len(want[0]) <= 16 and len(want[2]) <= 16 and len(want[1]) > 64
    out = torch.full((64,), 0xAB, dtype=torch.uint8, device="cuda")
    out, cur, tab = _placed(eng, masks, (5, 9, 64, 60), (130, 90), out=out)
    assert tab[1, 1] == -len(want[1]) - 1                            # the needed size, negated; the mask takes no room
    assert tab[0, 1] == len(want[0]) and tab[2, 1] == len(want[2])
    assert tab[0, 0] == 0 and tab[2, 0] == 16 and int(cur.item()) == 32
    got = _strings(out, tab[[0, 2]])
    assert got == [want[0], want[2]] and bool((out[32:] == 0xAB).all())


# ---- 3. - 5. the pipeline against a manual composition ---------------------------------------------------------------------------

EXAMPLE_BOXES = np.array([[10, 12, 60, 70], [180, 20, 250, 90], [230, 100, 330, 180], [650.5, 550.2, 699.9, 599.9],
                          [300, 300, 340, 330], [190, 190, 260, 260], [100, 100, 420, 380], [0, 0, 700, 600]], np.float32)
EXAMPLE_LABELS = np.array([3, 0, 7, 7, 12, 1, 5, 9], np.int64)


def _window_masks(sam, image, boxes, window, overlap, context=2.0):
    """What scene mode is specified to compute, by hand: per planned window SamPredictor.set_image(crop) and predict_torch with
    the window's boxes shifted by its origin -> [(masks uint8 [n, h, w], ranks, window)]."""
    import samrs_amd
    from samrs_amd.scene import plan_scene
    H, W = image.shape[:2]
    windows, window_of = plan_scene(H, W, boxes, window, overlap, context)
    pred = samrs_amd.SamPredictor(sam)
    parts = []
    for k, (x0, y0, w, h) in enumerate(windows):
        ranks = np.array([j for j, kk in enumerate(window_of) if kk == k], np.int32)
        pred.set_image(np.ascontiguousarray(image[y0:y0 + h, x0:x0 + w]))
        shifted = boxes[ranks] - np.array([x0, y0, x0, y0], np.float32)
        tb = pred.transform.apply_boxes_torch(torch.from_numpy(shifted).cuda(), (h, w))
        masks, _, _ = pred.predict_torch(None, None, tb, None, multimask_output=False)
        parts.append((masks[:, 0].cpu().numpy().astype(np.uint8), ranks, (x0, y0, w, h)))
    return windows, window_of, parts


def _expected(parts, labels, H, W):
    seg, areas = scene_ref.composite(parts, labels, H, W)
    rles = [None] * len(labels)
    for masks, ranks, (x0, y0, w, h) in parts:
        for m, r in zip(masks, ranks):
            rles[r] = scene_ref.scene_rle(m, x0, y0, H, W)
    return seg, areas, rles, scene_ref.class_stats(areas, labels, N_CLASSES)


@pytest.fixture(scope="module")
def example(sam):
    image = synth.make_image(31, 600, 700)
    windows, window_of, parts = _window_masks(sam, image, EXAMPLE_BOXES, 256, 64)
    assert len(windows) == 7
    return image, windows, window_of, parts


def _run_scene(pipe, items):
    got = {}

    def sink(results, release):
        for r in results:
            png = (bytes(r.png("gray")), bytes(r.png("color"))) if r.png_table is not None else None
            got[r.key] = (r, r.seg_mask.copy(), r.areas.copy(), [r.rle(j) for j in range(len(r.labels))] if r.rle_table is not None else None,
                          png)
        release()
    pipe.run(items, sink)
    return got, pipe.class_pixels.cpu().numpy(), pipe.class_instances.cpu().numpy()


@pytest.mark.parametrize("batching", [dict(), dict(batch=2, box_batch=3)])
def test_scene_pipeline_equals_the_manual_composition(sam, example, batching):
    from samrs_amd import driver
    from samrs_amd.scene import ScenePipeline
    image, windows, window_of, parts = example
    want_seg, want_areas, want_rles, (want_pix, want_ins) = _expected(parts, EXAMPLE_LABELS, 600, 700)
    pipe = ScenePipeline(sam, N_CLASSES, window=256, overlap=64, precision="engine", rle=True, rle_buffer_mb=16, **batching)
    got, pix, ins = _run_scene(pipe, [driver.WorkItem("scene", image, EXAMPLE_BOXES, EXAMPLE_LABELS)])
    r, seg, areas, rles, png = got["scene"]
    assert r.windows == windows and r.window_of == window_of and r.size == (600, 700) and png is None
    assert np.array_equal(r.boxes, EXAMPLE_BOXES) and np.array_equal(r.labels, EXAMPLE_LABELS)
    assert seg.shape == (600, 700) and np.array_equal(seg, want_seg)
    assert np.array_equal(areas, want_areas)
    assert rles == want_rles
    assert np.array_equal(pix, want_pix) and np.array_equal(ins, want_ins)


def test_scene_no_larger_than_the_window_equals_tile_pipeline(sam):
    from samrs_amd import driver
    from samrs_amd.scene import ScenePipeline
    items = []
    for i, ((h, w), n) in enumerate(zip([(1024, 1024), (800, 640)], [23, 9])):
        boxes, labels = synth.make_boxes(50 + i, n, h, w)
        items.append(driver.WorkItem(f"img{i}", synth.make_image(50 + i, h, w), boxes, labels))
    lut = tile_io.class_lut(np.random.default_rng(1).integers(0, 256, (N_CLASSES, 3), dtype=np.uint8))
    tile = driver.TilePipeline(sam, N_CLASSES, batch=2, box_batch=20, max_boxes=64, rle=True, rle_buffer_mb=16, png_lut=lut)
    want = {}

    def sink(results, release):
        for r in results:
            want[r.key] = (r.seg_mask.copy(), r.areas.copy(), [r.rle(j) for j in range(len(r.labels))], (bytes(r.png("gray")), bytes(r.png("color"))))
        release()
    tile.run(driver.batched(items, 2), sink)
    scene = ScenePipeline(sam, N_CLASSES, window=1024, batch=2, box_batch=20, rle=True, rle_buffer_mb=16, png_lut=lut)
    got, pix, ins = _run_scene(scene, items)
    for it in items:
        r, seg, areas, rles, png = got[it.key]
        h, w = it.image.shape[:2]
        assert r.windows == [(0, 0, w, h)] and set(r.window_of) == {0}
        assert seg.dtype == np.uint8 and seg.tobytes() == want[it.key][0].tobytes(), it.key
        assert np.array_equal(areas, want[it.key][1]), it.key
        assert rles == want[it.key][2], it.key
        assert png == want[it.key][3], it.key
    assert np.array_equal(pix, tile.class_pixels.cpu().numpy()) and np.array_equal(ins, tile.class_instances.cpu().numpy())


def test_scene_pipeline_with_the_small_region_cleanup(sam, example):
    from samrs_amd import driver
    from samrs_amd.scene import ScenePipeline
    image, windows, window_of, parts = example
    cleaned, changed = [], np.zeros(len(EXAMPLE_LABELS), np.int64)
    for masks, ranks, win in parts:
        c, _, chg = region_ref.clean_batch(masks, 16, "both")
        cleaned.append((c, ranks, win))
        changed[ranks] = chg
    want_seg, want_areas, want_rles, (want_pix, want_ins) = _expected(cleaned, EXAMPLE_LABELS, 600, 700)
    pipe = ScenePipeline(sam, N_CLASSES, window=256, overlap=64, precision="engine", rle=True, rle_buffer_mb=16, min_region_area=16)
    got, pix, ins = _run_scene(pipe, [driver.WorkItem("scene", image, EXAMPLE_BOXES, EXAMPLE_LABELS)])
    r, seg, areas, rles, _ = got["scene"]
    assert np.array_equal(seg, want_seg) and np.array_equal(areas, want_areas) and rles == want_rles
    assert np.array_equal(r.changed, changed)
    assert np.array_equal(pix, want_pix) and np.array_equal(ins, want_ins)


# ---- 6. the CLI -------------------------------------------------------------------------------------------------------------------

def test_cli_scene_window_writes_scene_frame_outputs(tmp_path):
    import samrs_amd
    from samrs_amd import driver, generate
    from samrs_amd.scene import ScenePipeline
    img_dir = tmp_path / "img"
    img_dir.mkdir()
    ann, scenes = {}, {}
    for i, (h, w) in enumerate([(300, 420), (500, 380)]):
        image = synth.make_image(80 + i, h, w)
        boxes, labels = synth.make_boxes(80 + i, 7, h, w)
        boxes = np.concatenate([boxes, np.array([[0, 0, w, h]], np.float32)])              # one box the size of the scene
        labels = np.concatenate([labels, [4]])
        tile_io.write_rgb(str(img_dir / f"S{i}.png"), image, 1)
        ann[f"S{i}"] = {"boxes": boxes.tolist(), "labels": [int(l) for l in labels]}
        scenes[f"S{i}"] = (image, boxes.astype(np.float32), labels.astype(np.int64))
    (tmp_path / "boxes.json").write_text(json.dumps(ann))
    out = tmp_path / "out"
    args = generate.build_parser().parse_args(["--images", str(img_dir), "--boxes", str(tmp_path / "boxes.json"), "--out", str(out),
                                               "--model", "vit_tiny", "--box-batch", "20", "--batch", "2", "--scene-window", "256",
                                               "--scene-overlap", "64"])
    stats = generate.run(args)
    assert os.path.exists(out / "statistic" / "class_stats.json") and os.path.exists(out / "statistic" / "all_mask_size.npy")
    # the same model as the CLI builds, the same pipeline, and the masks by hand
    sam = samrs_amd.sam_model_registry["vit_tiny"](checkpoint=None, precision="f16", options={"split": 15}, max_images=4,
                                                   max_prompts=20).to("cuda")
    pipe = ScenePipeline(sam, N_CLASSES, window=256, overlap=64, batch=2, box_batch=20, rle=True)
    got, pix, ins = _run_scene(pipe, [driver.WorkItem(k, *v) for k, v in scenes.items()])
    assert stats["class_pixel_num"] == pix.tolist() and stats["class_instance_num"] == ins.tolist()
    for stem, (image, boxes, labels) in scenes.items():
        H, W = image.shape[:2]
        r, seg, areas, rles, _ = got[stem]
        assert len(r.windows) > 1
        assert np.array_equal(tile_io.read_rgb(str(out / "gray" / f"{stem}.png"))[..., 0], seg)
        assert tile_io.read_rgb(str(out / "color" / f"{stem}.png")).shape == (H, W, 3)
        _, _, parts = _window_masks(sam, image, boxes, 256, 64)
        pasted = {int(rk): scene_ref.paste(m, win[0], win[1], H, W) for masks, ranks, win in parts for m, rk in zip(masks, ranks)}
        with open(out / "ins" / f"{stem}.pkl", "rb") as f:
            info = pickle.load(f)
        assert len(info) == len(labels)
        for j, entry in enumerate(info):
            assert list(entry["mask"]["size"]) == [H, W]
            assert np.array_equal(rle.decode(entry["mask"]), pasted[j]), (stem, j)
            assert entry["size"] == int(pasted[j].sum()) == int(areas[j]) and entry["label"] == int(labels[j])
