"""Host reference for ``samrs_resolve_overlaps`` (imported by tests/test_overlap_host.py and tests/test_overlap_gpu.py): numpy only.

The sequential rule of include/samrs_hip.h restated: walk the masks j = 0 .. n-1 and keep a holder per pixel.  Mask j is a candidate at
p iff its byte is set; it replaces holder b iff there is no holder, or P[j] > P[b], or P[j] == P[b] and not v_j(p) < v_b(p).  Ties
and non-comparable values go to the later mask.  Without logits the v term is absent (equal)."""
from typing import Optional, Tuple

import numpy as np

RULES = {"logit": 1, "smallest": 2, "priority": 3}


def primary(masks, rule: str, priority=None) -> np.ndarray:
    """int64 [n]: the primary key of every mask under `rule`."""
    m = np.asarray(masks) != 0
    if rule == "logit":
        return np.zeros(len(m), dtype=np.int64)
    if rule == "smallest":
        return -m.sum(axis=(1, 2)).astype(np.int64)
    if rule == "priority":
        return np.asarray(priority, dtype=np.int64)
    raise ValueError(rule)


def resolve(masks, logits: Optional[np.ndarray] = None, prim: Optional[np.ndarray] = None
            ) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """masks [n, H, W] (non-zero = set), logits fp32 [n, H, W] or None, prim int64 [n] or None (all equal) ->
    (disjoint masks, the winners' bytes as they were; owner int32 [H, W], -1 where no mask is set; before int64 [n]; removed int64 [n])."""
    m = np.asarray(masks)
    n = len(m)
    h, w = m.shape[1:] if n else (0, 0)
    P = np.zeros(n, dtype=np.int64) if prim is None else np.asarray(prim, dtype=np.int64)
    owner = np.full((h, w), -1, dtype=np.int32)
    pb = np.zeros((h, w), dtype=np.int64)
    vb = np.zeros((h, w), dtype=np.float32)
    for j in range(n):
        cand = m[j] != 0
        vj = np.zeros((h, w), dtype=np.float32) if logits is None else np.asarray(logits[j], dtype=np.float32)
        with np.errstate(invalid="ignore"):
            take = cand & ((owner < 0) | (P[j] > pb) | ((P[j] == pb) & ~(vj < vb)))
        owner[take] = j
        pb[take] = P[j]
        vb[take] = vj[take]
    out = m.copy()
    for j in range(n):
        out[j][owner != j] = 0
    before = (m != 0).sum(axis=(1, 2)).astype(np.int64)
    after = (out != 0).sum(axis=(1, 2)).astype(np.int64)
    return out, owner, before, before - after


def band(masks, logits: np.ndarray, tol: float, any_pair: bool = False) -> np.ndarray:
    """bool [H, W]: the contested pixels whose two best candidates' logits differ by <= tol -- where a logit that is off by tol may
    pick another winner (rule "logit").  any_pair: where ANY two candidates' logits are that close (a rule whose primary key decides
    which pair the logit separates)."""
    m = np.asarray(masks) != 0
    if len(m) < 2:
        return np.zeros(m.shape[1:], dtype=bool)
    v = np.sort(np.where(m, np.asarray(logits, dtype=np.float64), -np.inf), axis=0)
    with np.errstate(invalid="ignore"):
        gap = v[1:] - v[:-1]                                     # -inf - -inf = nan: not close
        close = (gap <= tol).any(0) if any_pair else gap[-1] <= tol
    return (m.sum(0) >= 2) & close


def paint(masks, labels) -> np.ndarray:
    """The class map painted in box order (a later box wins, 255 = unlabeled)."""
    m = np.asarray(masks) != 0
    seg = np.full(m.shape[1:], 255, dtype=np.uint8)
    for j in range(len(m)):
        seg[m[j]] = int(labels[j])
    return seg
