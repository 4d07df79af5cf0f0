"""Plain-numpy statement of COCO mask AP for one category without crowd annotations -- COCOeval.evaluateImg, accumulate and
summarize restated with sequential loops (pycocotools is not a dependency), written independently of samrs_amd/coco_ap.py and of the
kernels it drives: masks in, twelve numbers out.

A match is a match by INDEX (ground truth 0 can be matched; pycocotools tests the stored annotation id for truth and loses it).
"""
import numpy as np

THRESHOLDS = np.linspace(.5, .95, 10)
RECALLS = np.linspace(.0, 1.0, 101)
RANGES = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
MAX_DETS = (1, 10, 100)
NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR@1", "AR@10", "AR@100", "ARs", "ARm", "ARl")


def pack_bits(masks):
    """uint64 [n, ceil(h w / 64)]: pixel p (row-major) = bit p % 64 of word p / 64, tail bits zero."""
    m = np.asarray(masks)
    n = m.shape[0]
    flat = (m.reshape(n, -1) != 0)
    hw = flat.shape[1]
    words = (hw + 63) // 64
    out = np.zeros((n, words), dtype=np.uint64)
    for j in range(n):
        for p in np.flatnonzero(flat[j]):
            out[j, p // 64] |= np.uint64(1) << np.uint64(p % 64)
    return out


def pack_bits_fast(masks):
    """The same through numpy's packbits (little bit order, little-endian words); checked against pack_bits in the host tests."""
    m = np.asarray(masks)
    n = m.shape[0]
    flat = (m.reshape(n, -1) != 0)
    words = (flat.shape[1] + 63) // 64
    pad = np.zeros((n, words * 64), dtype=bool)
    pad[:, :flat.shape[1]] = flat
    return np.packbits(pad, axis=1, bitorder="little").view("<u8").astype(np.uint64).reshape(n, words)


def label_masks(label_rgb, colors):
    """bool [n, h, w]: instance j = the pixels whose RGB equals colors[j]."""
    lab, col = np.asarray(label_rgb), np.asarray(colors)
    return np.stack([np.all(lab == col[j][None, None, :], axis=2) for j in range(len(col))]) if len(col) else \
        np.zeros((0,) + lab.shape[:2], bool)


def pair_counts(a_masks, b_masks):
    """(inter int64 [na, nb], area_a, area_b) of two mask stacks."""
    a, b = np.asarray(a_masks), np.asarray(b_masks)
    hw = int(np.prod(a.shape[1:])) if len(a) else int(np.prod(b.shape[1:]))
    a = (a.reshape(len(a), hw) != 0).astype(np.int64)
    b = (b.reshape(len(b), hw) != 0).astype(np.int64)
    return a @ b.T, a.sum(1), b.sum(1)


def match_counts(inter, area_d, area_g, scores, thresholds=THRESHOLDS, ranges=RANGES, max_det=100):
    """evaluateImg from the integer counts -> dict(order [n_kept], match [A, T, max_det] (-1 = none), dt_ignore [A, T, max_det],
    n_valid [A], n_kept), padded like the device tables (ranks past n_kept: -1 / 0)."""
    scores = np.asarray(scores, dtype=np.float32)
    nd, ng = len(area_d), len(area_g)
    order = np.argsort(-scores, kind="mergesort")[:max_det]
    n_kept = len(order)
    A, T = len(ranges), len(thresholds)
    match = -np.ones((A, T, max_det), dtype=np.int32)
    ignore = np.zeros((A, T, max_det), dtype=np.uint8)
    n_valid = np.zeros(A, dtype=np.int32)
    iou = np.zeros((nd, ng), dtype=np.float64)
    for d in range(nd):
        for g in range(ng):
            union = int(area_d[d]) + int(area_g[g]) - int(inter[d][g])
            iou[d, g] = (np.float64(int(inter[d][g])) / np.float64(union)) if union > 0 else 0.0
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
    return {"order": order.astype(np.int32), "match": match, "dt_ignore": ignore, "n_valid": n_valid, "n_kept": n_kept,
            "scores": scores.astype(np.float64)}


def match_masks(pred_masks, scores, gt_masks, **kw):
    inter, ad, ag = pair_counts(pred_masks, gt_masks)
    return match_counts(inter, ad, ag, scores, **kw)


def accumulate_tables(tables, max_dets=MAX_DETS):
    """accumulate + summarize over per-image tables (match_counts' dicts) -> the twelve numbers by name."""
    A = len(RANGES) if not tables else len(tables[0]["n_valid"])
    T = len(THRESHOLDS) if not tables else np.asarray(tables[0]["match"]).shape[1]
    R, M = len(RECALLS), len(max_dets)
    precision = -np.ones((T, R, A, M))
    recall = -np.ones((T, A, M))
    for a in range(A):
        n_gt = 0
        for tb in tables:
            n_gt += int(tb["n_valid"][a])
        if n_gt == 0:
            continue
        for mi, m in enumerate(max_dets):
            rows = []                                   # (score, per-threshold matched, per-threshold ignored), image by image
            for tb in tables:
                k = min(m, int(tb["n_kept"]))
                for r in range(k):
                    d = int(tb["order"][r])
                    rows.append((float(tb["scores"][d]), [int(tb["match"][a][t][r]) >= 0 for t in range(T)],
                                 [bool(tb["dt_ignore"][a][t][r]) for t in range(T)]))
            idx = sorted(range(len(rows)), key=lambda i: -rows[i][0])          # Python's sort is stable
            for t in range(T):
                tp = fp = 0
                rc, pr = [], []
                for i in idx:
                    _, matched, ignored = rows[i]
                    if matched[t] and not ignored[t]:
                        tp += 1
                    if not matched[t] and not ignored[t]:
                        fp += 1
                    rc.append(np.float64(tp) / n_gt)
                    pr.append(np.float64(tp) / (np.float64(fp) + np.float64(tp) + np.spacing(1)))
                recall[t, a, mi] = rc[-1] if rc else 0
                for i in range(len(pr) - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                for ri, level in enumerate(RECALLS):
                    pi = 0
                    while pi < len(rc) and rc[pi] < level:
                        pi += 1
                    precision[t, ri, a, mi] = pr[pi] if pi < len(pr) else 0.0

    def mean(s):
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0
    out = {"AP": mean(precision[:, :, 0, M - 1]), "AP50": mean(precision[0, :, 0, M - 1]), "AP75": mean(precision[5, :, 0, M - 1]),
           "APs": mean(precision[:, :, 1, M - 1]), "APm": mean(precision[:, :, 2, M - 1]), "APl": mean(precision[:, :, 3, M - 1])}
    for mi, m in enumerate(max_dets):
        out[f"AR@{m}"] = mean(recall[:, 0, mi])
    out.update(ARs=mean(recall[:, 1, M - 1]), ARm=mean(recall[:, 2, M - 1]), ARl=mean(recall[:, 3, M - 1]))
    return out


def evaluate(images, max_dets=MAX_DETS):
    """images: (pred_masks, scores, gt_masks) per image -> (the twelve numbers, the per-image tables)."""
    tables = [match_masks(p, s, g, max_det=max(max_dets)) for p, s, g in images]
    return accumulate_tables(tables, max_dets), tables
