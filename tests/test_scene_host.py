"""CPU: scene mode's host side -- the window planner (samrs_amd.scene.plan_scene) against the rules it is specified by, the
three C-ABI declarations, and the generation CLI's flags.  No GPU."""
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _starts(L, window, overlap):
    """Rule 1 restated: the grid's starts along an axis."""
    if L <= window:
        return [0]
    out, s = [], 0
    while s + window < L:
        out.append(s)
        s += window - overlap
    return out + [L - window]


def _hull(box, H, W):
    x1, y1, x2, y2 = (float(v) for v in box)
    cx = lambda v: min(max(v, 0.0), float(W))
    cy = lambda v: min(max(v, 0.0), float(H))
    return math.floor(cx(x1)), math.floor(cy(y1)), math.ceil(cx(x2)), math.ceil(cy(y2))


def _contains(win, hull):
    x0, y0, w, h = win
    lx, ly, hx, hy = hull
    return x0 <= min(lx, hx) and max(lx, hx) <= x0 + w and y0 <= min(ly, hy) and max(ly, hy) <= y0 + h


def test_worked_example_window_for_window():
    from samrs_amd.scene import axis_spans, plan_scene
    H, W = 600, 700
    assert [s for s, _ in axis_spans(W, 256, 64)] == [0, 192, 384, 444]
    assert [s for s, _ in axis_spans(H, 256, 64)] == [0, 192, 344]
    boxes = [[10, 12, 60, 70], [180, 20, 250, 90], [230, 100, 330, 180], [650.5, 550.2, 699.9, 599.9], [300, 300, 340, 330],
             [190, 190, 260, 260], [100, 100, 420, 380], [0, 0, 700, 600]]
    windows, window_of = plan_scene(H, W, boxes, window=256, overlap=64)
    want = [(0, 0, 256, 256), (0, 0, 256, 256), (192, 0, 256, 256), (444, 344, 256, 256), (192, 192, 256, 256),
            (97, 97, 256, 256), (0, 0, 640, 600), (0, 0, 700, 600)]
    assert [windows[k] for k in window_of] == want
    assert len(windows) == 7
    assert windows == [(0, 0, 256, 256), (192, 0, 256, 256), (444, 344, 256, 256), (192, 192, 256, 256), (97, 97, 256, 256),
                       (0, 0, 640, 600), (0, 0, 700, 600)]                       # order of first use, identical windows shared
    assert all(isinstance(v, int) for win in windows for v in win)


def _random_boxes(rng, n, H, W):
    boxes = []
    for _ in range(n):
        kind = rng.integers(0, 6)
        if kind == 0:                                        # wholly outside the scene
            x, y = W + rng.uniform(1, 50), rng.uniform(-80, -10)
            boxes.append([x, y, x + rng.uniform(0, 40), y + rng.uniform(0, 5)])
        elif kind == 1:                                      # zero size
            x, y = rng.uniform(0, W), rng.uniform(0, H)
            boxes.append([x, y, x, y])
        elif kind == 2:                                      # partly outside
            x, y = rng.uniform(-60, W), rng.uniform(-60, H)
            boxes.append([x, y, x + rng.uniform(1, 300), y + rng.uniform(1, 300)])
        else:
            bw, bh = np.exp(rng.uniform(np.log(2), np.log(max(3, W)))), np.exp(rng.uniform(np.log(2), np.log(max(3, H))))
            x, y = rng.uniform(0, W), rng.uniform(0, H)
            boxes.append([x - bw / 2, y - bh / 2, x + bw / 2, y + bh / 2])
    return np.asarray(boxes, dtype=np.float32).reshape(-1, 4)


@pytest.mark.parametrize("seed", range(8))
def test_planner_properties_on_random_scenes(seed):
    from samrs_amd.scene import plan_scene
    rng = np.random.default_rng(100 + seed)
    for _ in range(40):
        H, W = int(rng.integers(50, 3001)), int(rng.integers(50, 3001))
        window = int(rng.choice([128, 256, 1024]))
        overlap = int(rng.choice([0, 32, 100]))
        context = float(rng.choice([1.0, 1.5, 2.0]))
        boxes = _random_boxes(rng, int(rng.integers(0, 31)), H, W)
        windows, window_of = plan_scene(H, W, boxes, window, overlap, context)
        assert plan_scene(H, W, boxes.copy(), window, overlap, context) == (windows, window_of)          # deterministic
        assert len(window_of) == len(boxes)                                                              # one window per box
        assert sorted(set(window_of)) == list(range(len(windows)))                                       # no window without a box
        assert len(set(windows)) == len(windows)                                                         # identical ones shared
        first_use = [window_of.index(k) for k in range(len(windows))]
        assert first_use == sorted(first_use)                                                            # in order of first use
        grid = [(x0, y0, min(window, W), min(window, H)) for y0 in _starts(H, window, overlap) for x0 in _starts(W, window, overlap)]
        for box, k in zip(boxes, window_of):
            x0, y0, w, h = win = windows[k]
            hull = _hull(box, H, W)
            assert 0 <= x0 and 0 <= y0 and w >= 1 and h >= 1 and x0 + w <= W and y0 + h <= H, (win, H, W)
            assert _contains(win, hull), (box, hull, win)
            holding = [g for g in grid if _contains(g, hull)]
            if holding:                                      # a grid window: side min(window, L), the greatest margin, first on ties
                assert win in holding and (w, h) == (min(window, W), min(window, H))
                lx, ly, hx, hy = hull
                margin = lambda g: min(lx - g[0], ly - g[1], g[0] + g[2] - hx, g[1] + g[3] - hy)
                assert win == max(holding, key=margin)       # max() returns the first of equal keys
            else:                                            # its own context window
                lx, ly, hx, hy = hull
                s = max(window, math.ceil(context * max(hx - lx, hy - ly)))
                assert (w, h) == (min(s, W), min(s, H))


def test_small_scene_no_boxes_and_bad_overlap():
    from samrs_amd.scene import plan_scene
    assert plan_scene(600, 800, [[5, 5, 50, 50], [700, 500, 799, 599]], window=1024) == ([(0, 0, 800, 600)], [0, 0])
    assert plan_scene(1024, 1024, [[0, 0, 1024, 1024]], window=1024) == ([(0, 0, 1024, 1024)], [0])
    assert plan_scene(4096, 4096, np.zeros((0, 4), np.float32)) == ([], [])
    assert plan_scene(4096, 4096, []) == ([], [])
    for overlap in (256, 300, -1):
        with pytest.raises(ValueError):
            plan_scene(2000, 2000, [[1, 1, 5, 5]], window=256, overlap=overlap)


def test_header_declares_the_scene_entry_points_and_abi_stays_5():
    text = open(os.path.join(ROOT, "include", "samrs_hip.h")).read()
    assert re.search(r"#define\s+SAMRS_ABI_VERSION\s+5\b", text)
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_params in (("samrs_scene_claim", 17), ("samrs_scene_resolve", 8), ("samrs_rle_encode_placed", 14)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == n_params, name
    from samrs_amd import engine
    assert engine.ABI_VERSION == 5
    src = open(os.path.join(ROOT, "samrs_amd", "csrc", "Makefile")).read()
    assert "scene_kernels.hip" in src


def test_generate_parser_has_the_scene_flags():
    from samrs_amd import generate
    ap = generate.build_parser()
    base = ["--images", "i", "--boxes", "b", "--out", "o"]
    ns = ap.parse_args(base)
    assert (ns.scene_window, ns.scene_overlap, ns.scene_context) == (0, 256, 2.0)
    ns = ap.parse_args(base + ["--scene-window", "512", "--scene-overlap", "64", "--scene-context", "1.5", "--png-device", "--resume",
                               "--no-rle", "--min-region-area", "16"])
    assert (ns.scene_window, ns.scene_overlap, ns.scene_context) == (512, 64, 1.5)
    assert ap.parse_args(base + ["--batch-decode"]).batch_decode                       # without scene mode the flag stands
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--scene-window", "512", "--batch-decode"])
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--scene-window", "256", "--scene-overlap", "256"])
