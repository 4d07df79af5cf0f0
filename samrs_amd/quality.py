"""Host helpers for the mask-quality counts of ``Engine.score_masks`` (samrs_score_masks): numpy only, nothing touches the device.

counts is int64 [n, 4] = n_hi, n_mid, n_lo, n_in: the output pixels whose logit is > +offset, > 0, > -offset, and > 0 inside the box
that prompted the mask.  ``keep_rule`` restates, in numpy, the rule ``Engine.filter_masks`` (samrs_filter_masks) applies on the
device: the thresholds are fp32 values compared in fp64 against the integer counts, so both sides decide every case alike."""
from __future__ import annotations

from typing import Optional

import numpy as np


def _counts(counts) -> np.ndarray:
    c = np.asarray(counts, dtype=np.int64)
    if c.ndim != 2 or c.shape[1] != 4:
        raise ValueError(f"counts must be [n, 4] (n_hi, n_mid, n_lo, n_in), got {c.shape}")
    return c


def stability(counts) -> np.ndarray:
    """``calculate_stability_score`` (utils/amg.py:156-176): n_hi / n_lo as float64 [n]; 0 / 0 -> 0.0 (the reference's NaN)."""
    c = _counts(counts)
    hi, lo = c[:, 0].astype(np.float64), c[:, 2].astype(np.float64)
    return np.where(lo > 0, hi / np.maximum(lo, 1.0), 0.0)


def inside_fraction(counts) -> np.ndarray:
    """The share of each mask inside the box that prompted it: n_in / n_mid as float64 [n]; an empty mask -> 1.0 (nothing leaks)."""
    c = _counts(counts)
    inside, mid = c[:, 3].astype(np.float64), c[:, 1].astype(np.float64)
    return np.where(mid > 0, inside / np.maximum(mid, 1.0), 1.0)


def keep_rule(counts, iou: Optional[np.ndarray] = None, min_stability: float = 0.0, min_pred_iou: float = 0.0,
              min_inside_box: float = 0.0) -> np.ndarray:
    """bool [n]: every enabled criterion holds (a threshold <= 0 disables its criterion, amg.py:295,303).  Each threshold is
    rounded to fp32 first -- the C ABI takes floats -- and the comparisons are made in fp64:
      stability      n_lo > 0 and n_hi >= min_stability * n_lo      (>= as the reference; 0 / 0 fails)
      predicted IoU  iou > min_pred_iou                             (strict as the reference; iou is fp32)
      box fit        n_mid == 0 or n_in >= min_inside_box * n_mid   (an empty mask passes)"""
    c = _counts(counts)
    hi, mid, lo, inside = (c[:, k].astype(np.float64) for k in range(4))
    ts, tq, tb = (np.float64(np.float32(t)) for t in (min_stability, min_pred_iou, min_inside_box))
    keep = np.ones(len(c), dtype=bool)
    if ts > 0:
        keep &= (lo > 0) & (hi >= ts * lo)
    if tq > 0:
        if iou is None:
            raise ValueError("min_pred_iou > 0 needs iou")
        q = np.asarray(iou, dtype=np.float32).reshape(-1)
        if q.shape[0] != len(c):
            raise ValueError(f"iou has {q.shape[0]} entries for {len(c)} masks")
        keep &= q > np.float32(min_pred_iou)
    if tb > 0:
        keep &= (mid == 0) | (inside >= tb * mid)
    return keep
