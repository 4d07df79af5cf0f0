"""Host restatement (numpy) of scene-mode compositing (samrs_scene_claim / samrs_scene_resolve / samrs_rle_encode_placed): masks
decoded in windows of a scene, pasted into the scene's frame and painted in annotation order, a later box winning
(Generate Dataset/main_sam_hbox_semantic.py:162,195-199).  Integer work on both sides: every comparison against it is exact."""
import numpy as np

from samrs_amd import rle


def paste(mask: np.ndarray, x0: int, y0: int, H: int, W: int) -> np.ndarray:
    """mask [h, w] (non-zero = set) at (x0, y0) on an all-zero bool [H, W] canvas."""
    h, w = mask.shape
    assert 0 <= x0 and 0 <= y0 and x0 + w <= W and y0 + h <= H
    out = np.zeros((H, W), dtype=bool)
    out[y0:y0 + h, x0:x0 + w] = np.asarray(mask) != 0
    return out


def composite(parts, labels, H: int, W: int):
    """parts: list of (masks [n, h, w], ranks [n], (x0, y0, w, h)); labels[r] = class of annotation r -> (seg uint8 [H, W] with
    255 = unlabeled, areas int64 [len(labels)]): every mask pasted, then painted in rank order."""
    seg = np.full((H, W), 255, dtype=np.uint8)
    areas = np.zeros(len(labels), dtype=np.int64)
    by_rank = {}
    for masks, ranks, (x0, y0, w, h) in parts:
        assert tuple(masks.shape[1:]) == (h, w)
        for m, r in zip(masks, ranks):
            assert int(r) not in by_rank
            by_rank[int(r)] = paste(m, x0, y0, H, W)
    for r in sorted(by_rank):
        seg[by_rank[r]] = np.uint8(labels[r])
        areas[r] = int(by_rank[r].sum())
    return seg, areas


def class_stats(areas, labels, n_classes: int):
    """statistic.py:18-21: pixels and instances per class over the instances with area > 0."""
    pix, ins = np.zeros(n_classes, np.int64), np.zeros(n_classes, np.int64)
    for a, l in zip(areas, labels):
        if a > 0 and 0 <= l < n_classes:
            pix[l] += int(a)
            ins[l] += 1
    return pix, ins


def scene_rle(mask: np.ndarray, x0: int, y0: int, H: int, W: int) -> dict:
    return rle.encode(paste(mask, x0, y0, H, W))
