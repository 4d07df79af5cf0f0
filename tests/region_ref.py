"""Host restatement of the small-region removal that ``samrs_clean_masks`` runs on the device (imported by
tests/test_clean_masks_host.py and tests/test_clean_masks_gpu.py).  numpy only.

Semantics (``remove_small_regions`` of the reference's ``segment_anything/utils/amg.py``, per pixel): a region is an 8-connected
component and is small when it has fewer than ``min_area`` pixels.

* ``"holes"``   -- every unset pixel in a small component of the complement becomes set;
* ``"islands"`` -- every set pixel in a small component is cleared; if every component is small exactly one stays, the largest,
  and among equally large ones the one whose first pixel in row-major order comes first;
* ``"both"``    -- holes, then islands on the result.

Labelling: union-find over the horizontal runs of the working set, which is fast in plain Python because blob-plus-speckle masks
have few runs.  Runs are numbered in row-major order and a union keeps the smaller number, so a component's root run is the run
that holds its first pixel in row-major order.
"""
import numpy as np

MODES = {"holes": 1, "islands": 2, "both": 3}


def _runs(work: np.ndarray):
    """Horizontal runs of a bool [h, w] array in row-major order: (row, first column, end column (exclusive))."""
    h, w = work.shape
    p = np.zeros((h, w + 2), dtype=np.int8)
    p[:, 1:-1] = work
    d = np.diff(p, axis=1)
    ys, s = np.nonzero(d == 1)
    _, e = np.nonzero(d == -1)
    return ys, s, e


def components(work: np.ndarray):
    """(row, start, end, root) per run: root = number of the first run (row-major) of the run's 8-connected component."""
    work = np.asarray(work).astype(bool)
    h = work.shape[0]
    ys, s, e = _runs(work)
    n = len(ys)
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    first = np.searchsorted(ys, np.arange(h + 1)).tolist()
    sl, el = s.tolist(), e.tolist()
    for y in range(1, h):
        a, a1, b, b1 = first[y - 1], first[y], first[y], first[y + 1]
        while a < a1 and b < b1:
            if sl[a] <= el[b] and sl[b] <= el[a]:          # columns overlap or touch diagonally
                ra, rb = find(a), find(b)
                if ra < rb:
                    parent[rb] = ra
                elif rb < ra:
                    parent[ra] = rb
            if el[a] < el[b]:
                a += 1
            else:
                b += 1
    root = np.fromiter((find(i) for i in range(n)), dtype=np.int64, count=n)
    return ys, s, e, root


def labels(mask: np.ndarray, complement: bool = False) -> np.ndarray:
    """int32 [h, w]: the smallest row-major pixel index of every pixel's component of the set (complement: unset) pixels, -1
    outside that working set."""
    work = (np.asarray(mask) != 0) != bool(complement)
    h, w = work.shape
    ys, s, e, root = components(work)
    out = np.full(h * w, -1, dtype=np.int32)
    first_pixel = ys * w + s
    out[np.flatnonzero(work.ravel())] = np.repeat(first_pixel[root], e - s) if len(ys) else 0
    return out.reshape(h, w)


def _small_pass(mask: np.ndarray, min_area: int, holes: bool) -> np.ndarray:
    """One pass on a bool [h, w] mask -> bool [h, w]."""
    work = ~mask if holes else mask
    ys, s, e, root = components(work)
    if len(ys) == 0:
        return mask.copy()
    lens = e - s
    area = np.bincount(root, weights=lens, minlength=len(ys)).astype(np.int64)       # per root run, 0 elsewhere
    small = area[root] < min_area                                                    # per run
    if holes:
        flip = small
    else:
        if not small.any():
            return mask.copy()
        if small.all():                      # keep the largest; np.argmax returns the first maximum = the first in row-major order
            flip = root != int(np.argmax(area))
        else:
            flip = small
    out = mask.copy().ravel()
    idx = np.flatnonzero(work.ravel())       # the working set's pixels in row-major order = run after run
    out[idx[np.repeat(flip, lens)]] = holes
    return out.reshape(mask.shape)


def clean(mask: np.ndarray, min_area: int, mode="both"):
    """mask [h, w] (non-zero = set) -> (cleaned uint8 [h, w] of 0 / 1, pixels set, pixels whose value changed)."""
    code = MODES[mode] if isinstance(mode, str) else int(mode)
    if min_area < 1 or code not in (1, 2, 3):
        raise ValueError("min_area >= 1 and mode holes / islands / both")
    src = np.asarray(mask) != 0
    out = src
    if code & 1:
        out = _small_pass(out, min_area, True)
    if code & 2:
        out = _small_pass(out, min_area, False)
    return out.astype(np.uint8), int(out.sum()), int((out != src).sum())


def clean_batch(masks: np.ndarray, min_area: int, mode="both"):
    """[n, h, w] -> (uint8 [n, h, w], areas int64 [n], changed int64 [n])."""
    res = [clean(m, min_area, mode) for m in masks]
    if not res:
        return np.zeros(np.shape(masks), np.uint8), np.zeros(0, np.int64), np.zeros(0, np.int64)
    return (np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int64),
            np.array([r[2] for r in res], dtype=np.int64))


def speckled_ellipse(seed: int, h: int = 1024, w: int = 1024, holes: float = 0.01, speckle: float = 0.003) -> np.ndarray:
    """The shape a SAM mask has: one blob with pin-holes inside it and stray pixels outside it (uint8 0 / 1)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = h * (0.4 + 0.2 * rng.random()), w * (0.4 + 0.2 * rng.random())
    ry, rx = h * (0.2 + 0.15 * rng.random()), w * (0.2 + 0.15 * rng.random())
    inside = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    noise = rng.random((h, w))
    return np.where(inside, noise >= holes, noise < speckle).astype(np.uint8)
