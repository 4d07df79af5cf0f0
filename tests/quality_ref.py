"""Host reference for the mask-quality counts of ``samrs_score_masks`` (imported by tests/test_quality_host.py and
tests/test_quality_gpu.py).  torch on the CPU only.

The logits reference is the reference's own postprocessing, ``F.interpolate`` -> crop -> ``F.interpolate`` (modeling/sam.py:133-162),
exactly as tests/test_kernels_gpu.py::test_postprocess_matches_interpolate builds it.  The device evaluates the same bilinear
formula with its own roundings; that test bounds the difference of the two logit maps by 1e-5, so a count against a threshold t may
differ by the pixels whose reference logit lies within 1e-5 of t and by no others: the `band`."""
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

LOGIT_TOL = 1e-5          # test_postprocess_matches_interpolate's bound on |device logit - host logit|

# the shapes the kernel-level tests share: (input size, original size), what each exercises
SHAPES = [
    ((1024, 1024), (1024, 1024)),      # the 4-pixel fast path
    ((1024, 768), (800, 600)),         # two-stage path, W % 4 == 0
    ((683, 1024), (1365, 2048)),       # upsampling; more pixels than one grid pass
    ((1024, 1024), (67, 93)),          # W % 4 != 0; partial waves; fewer pixels than one block's stride
    ((1024, 1024), (1, 1)),            # degenerate
]
OFFSETS = [1.0, 0.25]


def make_low(n: int = 3, seed: int = 3) -> torch.Tensor:
    """low = 4 * randn(n, 256, 256), generator seed 3: logits with SAM's spread, every threshold crossed often."""
    g = torch.Generator().manual_seed(seed)
    return 4.0 * torch.randn(n, 256, 256, generator=g)


def logits(low: torch.Tensor, input_size: Sequence[int], original_size: Sequence[int], img_size: int = 1024) -> torch.Tensor:
    """low fp32 [n, 256, 256] -> the reference's full-resolution logits fp32 [n, H, W]."""
    ref = F.interpolate(low[None].float(), (img_size, img_size), mode="bilinear", align_corners=False)
    ref = ref[..., : int(input_size[0]), : int(input_size[1])]
    return F.interpolate(ref, tuple(int(v) for v in original_size), mode="bilinear", align_corners=False)[0]


def inside_box(h: int, w: int, boxes) -> torch.Tensor:
    """bool [n, h, w]: bx0 <= (float)x <= bx1 and by0 <= (float)y <= by1 in fp32, per box (xyxy)."""
    b = torch.as_tensor(np.asarray(boxes, dtype=np.float32)).reshape(-1, 4)
    x = torch.arange(w, dtype=torch.float32)[None, None, :]
    y = torch.arange(h, dtype=torch.float32)[None, :, None]
    return (b[:, 0, None, None] <= x) & (x <= b[:, 2, None, None]) & (b[:, 1, None, None] <= y) & (y <= b[:, 3, None, None])


def counts(ref: torch.Tensor, offset: float, boxes=None) -> Tuple[np.ndarray, np.ndarray]:
    """ref fp32 [n, H, W] -> (counts int64 [n, 4] = n_hi, n_mid, n_lo, n_in; band int64 [n, 3] = pixels within LOGIT_TOL of
    +offset, 0, -offset).  n_in is 0 without boxes."""
    n, h, w = ref.shape
    off = float(np.float32(offset))
    out = np.zeros((n, 4), dtype=np.int64)
    band = np.zeros((n, 3), dtype=np.int64)
    for k, t in enumerate((off, 0.0, -off)):
        out[:, k] = (ref > t).flatten(1).sum(1).numpy()
        band[:, k] = ((ref - t).abs() <= LOGIT_TOL).flatten(1).sum(1).numpy()
    if boxes is not None:
        out[:, 3] = ((ref > 0) & inside_box(h, w, boxes)).flatten(1).sum(1).numpy()
    return out, band


def inside_count(masks, boxes) -> np.ndarray:
    """int64 [n]: the set pixels of masks [n, H, W] (non-zero = set) inside their boxes."""
    m = torch.as_tensor(np.asarray(masks)) != 0
    return (m & inside_box(m.shape[1], m.shape[2], boxes)).flatten(1).sum(1).numpy().astype(np.int64)


def stability_score(masks: torch.Tensor, mask_threshold: float, threshold_offset: float) -> torch.Tensor:
    """``calculate_stability_score`` (utils/amg.py:156-176) restated: masks = logits [..., H, W] -> intersections / unions."""
    inter = (masks > (mask_threshold + threshold_offset)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    union = (masks > (mask_threshold - threshold_offset)).sum(-1, dtype=torch.int16).sum(-1, dtype=torch.int32)
    return inter / union


def repaint(masks, labels, keep: Optional[np.ndarray] = None) -> np.ndarray:
    """The class map a host loop paints from masks [n, H, W] in box order (a later box wins, 255 = unlabeled,
    main_sam_hbox_semantic.py:162,195-199), from the kept masks only."""
    m = np.asarray(masks) != 0
    seg = np.full(m.shape[1:], 255, dtype=np.uint8)
    for j in range(len(m)):
        if keep is None or keep[j]:
            seg[m[j]] = int(labels[j])
    return seg
