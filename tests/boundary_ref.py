"""Plain-numpy statement of the boundary band, Boundary IoU and Boundary AP's matching (Cheng et al., CVPR 2021), with sequential
loops, written independently of samrs_amd/coco_ap.py and of the kernels: masks in, integer counts and tables out.

    band(M)      = M and not erode^d(M): d literal 3 x 3 all-ones erosions on a zero-padded copy (everything outside the image is
                   background), so the band holds the set pixels within Chebyshev distance d of a background pixel or the image edge.
    boundary IoU = |band(P) and band(G)| / |band(P) or band(G)|, 0 for an empty union.
    matching     = coco_ap_ref.match_counts' loop with the pair score min(mask IoU, boundary IoU); area ranges and ignore flags
                   still look at the MASK areas.

The matching loop is ``match_iou`` below: coco_ap_ref.match_counts with the IoU matrix as an argument (that function computes its
own from the counts and cannot be handed one); the host tests hold the two equal on mask IoU, so only the matrix differs.
"""
import math

import numpy as np

from coco_ap_ref import MAX_DETS, RANGES, THRESHOLDS, accumulate_tables, pair_counts


def dilation(h, w, ratio=0.02):
    return max(1, int(round(ratio * math.hypot(h, w))))


def erode3(mask):
    """One 3 x 3 all-ones erosion with a zero border."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    pad = np.zeros((h + 2, w + 2), dtype=bool)
    pad[1:-1, 1:-1] = m
    out = np.ones((h, w), dtype=bool)
    for dy in range(3):
        for dx in range(3):
            out &= pad[dy:dy + h, dx:dx + w]
    return out


def band(mask, d):
    """bool [h, w]: the mask minus its d-fold 3 x 3 erosion."""
    m = np.asarray(mask) != 0
    e = m
    for _ in range(int(d)):
        e = erode3(e)
    return m & ~e


def band_window(mask, d):
    """The same by the (2 d + 1)^2-window form, pixel by pixel: E[y][x] = 1 iff the whole square is inside the image and set."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    e = np.zeros((h, w), dtype=bool)
    for y in range(d, h - d):
        for x in range(d, w - d):
            e[y, x] = bool(m[y - d:y + d + 1, x - d:x + d + 1].all())
    return m & ~e


def bands(masks, d):
    m = np.asarray(masks)
    return np.stack([band(x, d) for x in m]) if len(m) else np.zeros(m.shape, dtype=bool)


def iou_matrix(inter, area_a, area_b):
    """float64 [na, nb]: inter / union as one IEEE division of the two integers, 0 for an empty union."""
    out = np.zeros((len(area_a), len(area_b)), dtype=np.float64)
    for i in range(len(area_a)):
        for j in range(len(area_b)):
            union = int(area_a[i]) + int(area_b[j]) - int(inter[i][j])
            out[i, j] = (np.float64(int(inter[i][j])) / np.float64(union)) if union > 0 else 0.0
    return out


def boundary_iou(pred, gt, d):
    i, a, b = pair_counts(band(pred, d)[None], band(gt, d)[None])
    return float(iou_matrix(i, a, b)[0, 0])


def match_iou(iou, area_d, area_g, scores, thresholds=THRESHOLDS, ranges=RANGES, max_det=100):
    """coco_ap_ref.match_counts' evaluateImg from a given IoU matrix [nd, ng] and the MASK areas."""
    scores = np.asarray(scores, dtype=np.float32)
    ng = len(area_g)
    order = np.argsort(-scores, kind="mergesort")[:max_det]
    A, T = len(ranges), len(thresholds)
    match = -np.ones((A, T, max_det), dtype=np.int32)
    ignore = np.zeros((A, T, max_det), dtype=np.uint8)
    n_valid = np.zeros(A, dtype=np.int32)
    for a, (lo, hi) in enumerate(ranges):
        g_ign = [bool(area_g[g] < lo or area_g[g] > hi) for g in range(ng)]
        visit = [g for g in range(ng) if not g_ign[g]] + [g for g in range(ng) if g_ign[g]]
        n_valid[a] = sum(1 for g in range(ng) if not g_ign[g])
        for t, thr in enumerate(thresholds):
            taken = [False] * ng
            for r, d in enumerate(order):
                best = min(float(thr), 1 - 1e-10)
                m = -1
                for g in visit:
                    if taken[g]:
                        continue
                    if m > -1 and not g_ign[m] and g_ign[g]:
                        break
                    if iou[d, g] < best:
                        continue
                    best = iou[d, g]
                    m = g
                if m > -1:
                    taken[m] = True
                    match[a, t, r] = m
                    ignore[a, t, r] = 1 if g_ign[m] else 0
                else:
                    ignore[a, t, r] = 1 if (area_d[d] < lo or area_d[d] > hi) else 0
    return {"order": order.astype(np.int32), "match": match, "dt_ignore": ignore, "n_valid": n_valid, "n_kept": len(order),
            "scores": scores.astype(np.float64)}


def match_counts_min(inter, area_d, area_g, inter_b, area_db, area_gb, scores, **kw):
    """Boundary AP's matching from the two triples of counts."""
    iou = np.minimum(iou_matrix(inter, area_d, area_g), iou_matrix(inter_b, area_db, area_gb))
    return match_iou(iou, area_d, area_g, scores, **kw)


def match_masks_min(pred_masks, scores, gt_masks, d, **kw):
    inter, ad, ag = pair_counts(pred_masks, gt_masks)
    ib, adb, agb = pair_counts(bands(pred_masks, d), bands(gt_masks, d))
    return match_counts_min(inter, ad, ag, ib, adb, agb, scores, **kw)


def evaluate(images, ratio=0.02, max_dets=MAX_DETS):
    """images: (pred_masks [nd, h, w], scores, gt_masks [ng, h, w]) per image -> (the twelve Boundary AP numbers, the tables)."""
    tables = []
    for p, s, g in images:
        h, w = (np.asarray(p).shape[1:] if len(p) else np.asarray(g).shape[1:])
        tables.append(match_masks_min(p, s, g, dilation(h, w, ratio), max_det=max(max_dets)))
    return accumulate_tables(tables, max_dets), tables


def boundary_miou(preds, gts, d):
    """(average, area) over the objects j = (preds[j], gts[j]) with a non-empty MASK union."""
    ious, si, su = [], 0, 0
    for p, g in zip(preds, gts):
        if not (np.asarray(p).any() or np.asarray(g).any()):
            continue
        bp, bg = band(p, d), band(g, d)
        i, u = int((bp & bg).sum()), int((bp | bg).sum())
        ious.append(i / u if u else 0.0)
        si += i
        su += u
    return (float(np.mean(ious)) if ious else 0.0), (si / su if su else 0.0)
