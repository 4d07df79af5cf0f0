"""The rule of samrs_fill_polygons (include/samrs_hip.h) as a plain per-pixel crossing count over Python ints: no numpy arithmetic, no
ceiling, no cumulative sum -- written independently of ``samrs_amd.polygons.rasterize_any``, which states the same rule edge by edge.

Pixel (r, c) of an h x w window whose origin is (x0, y0) has its centre at (c + 1/2, r + 1/2).  An edge (xa, ya) -> (xb, yb) of a
ring (the last vertex closes on the first; (x0, y0) subtracted) with dy = yb - ya != 0 counts for the pixel when
    min(ya, yb) <= r < max(ya, yb)                      (the centre's row line crosses it; vertices are integers, so never at a vertex)
and the centre is at or right of the crossing X = xa + dx (2 r + 1 - 2 ya) / (2 dy), that is 2 c + 1 >= 2 X, which multiplied by
dy reads
    (2 c + 1 - 2 xa) dy >= dx (2 r + 1 - 2 ya)          for dy > 0,
    (2 c + 1 - 2 xa) dy <= dx (2 r + 1 - 2 ya)          for dy < 0.
The pixel is 1 iff an odd number of the edges of all rings of the row count for it."""
from typing import Optional, Sequence

import numpy as np

REACH = 1 << 20         # a vertex farther than this from the origin in a coordinate: the row is not rings


def edges_of(rings_list: Sequence, x0: int = 0, y0: int = 0):
    """[(xa, ya, xb, yb)] of every ring of one row, as Python ints in the window's frame"""
    out = []
    for ring in rings_list:
        pts = ring[0] if isinstance(ring, tuple) else ring
        p = [(int(x) - x0, int(y) - y0) for x, y in np.asarray(pts).reshape(-1, 2).tolist()]
        for i, (xa, ya) in enumerate(p):
            xb, yb = p[(i + 1) % len(p)]
            out.append((xa, ya, xb, yb))
    return out


def pixel(edges, r: int, c: int) -> int:
    n = 0
    for xa, ya, xb, yb in edges:
        dx, dy = xb - xa, yb - ya
        if dy == 0 or not (min(ya, yb) <= r < max(ya, yb)):
            continue
        lhs, rhs = (2 * c + 1 - 2 * xa) * dy, dx * (2 * r + 1 - 2 * ya)
        if (lhs >= rhs) if dy > 0 else (lhs <= rhs):
            n += 1
    return n & 1


def placed(rings_list: Optional[Sequence], x0: int = 0, y0: int = 0) -> bool:
    """a row the library fills: rings (not None), every vertex within REACH of the origin"""
    if rings_list is None:
        return False
    return all(abs(v) <= REACH for e in edges_of(rings_list, x0, y0) for v in e)


def fill(rings_list: Optional[Sequence], h: int, w: int, origin=(0, 0)) -> np.ndarray:
    """uint8 [h, w]; a row that is not rings fills as empty"""
    x0, y0 = int(origin[0]), int(origin[1])
    out = np.zeros((h, w), np.uint8)
    if not placed(rings_list, x0, y0):
        return out
    edges = edges_of(rings_list, x0, y0)
    for r in range(h):
        row = [e for e in edges if e[1] != e[3] and min(e[1], e[3]) <= r < max(e[1], e[3])]
        if row:
            for c in range(w):
                out[r, c] = pixel(row, r, c)
    return out


def counts(filled: np.ndarray, ref: Optional[np.ndarray], is_rings: bool = True):
    """(fill, ref, both) as the library reports them: fill = -1 for a row that is not rings, the last two 0 without ref"""
    f = int(filled.sum()) if is_rings else -1
    if ref is None:
        return [f, 0, 0]
    g = np.asarray(ref) != 0
    return [f, int(g.sum()), int((g & (filled != 0)).sum())]
