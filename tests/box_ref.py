"""Host restatement of the mask-derived boxes that ``samrs_mask_boxes`` computes on the device (imported by
tests/test_mask_boxes_host.py, tests/test_mask_boxes_gpu.py and tools/mask_boxes_bench.py).  numpy and Python integers only.

Definition (the header comment of samrs_amd/csrc/box_kernels.hip states the same):
  points      the set pixels of a mask as integer points (x0 + col, y0 + row): pixel CENTRES, the convention of
              cv2.findContours -> cv2.minAreaRect and the frame the reference's rbox polygons are stated in;
  hbox        (xmin, ymin, xmax, ymax), inclusive integers;
  hull        the strict vertices of the convex hull (no collinear points), from v0 = the set pixel with the smallest (y, x): down
              the left side to the leftmost pixel of the last non-empty row, along that row to its rightmost pixel, up the right
              side to the rightmost pixel of the first non-empty row, back to v0; a repeated point appears once.  m vertices
              (1 for one pixel, 2 for collinear pixels);
  candidates  edge k runs from vertex k to vertex (k + 1) mod m; (dx, dy) = v[k + 1] - v[k], not reduced by the gcd.  Over the hull
              vertices p = x dx + y dy, q = -x dy + y dx; the candidate's rectangle has area (pmax - pmin)(qmax - qmin) / (dx^2 + dy^2),
              an exact rational;
  winner      the smallest area, compared exactly; ties go to the smallest k.  m = 1: (dx, dy) = (1, 0);
  corners     (pmin, qmin), (pmax, qmin), (pmax, qmax), (pmin, qmax) with x = (p dx - q dy) / L, y = (p dy + q dx) / L, L = dx^2 + dy^2:
              the integer numerator (below 2^53) converted to fp64, divided once, rounded to fp32;
  record      int64 [8]: dx, dy, pmin, pmax, qmin, qmax, m, and twice the hull's area = sum over the ordered vertices of
              x[k + 1] y[k] - x[k] y[k + 1] (>= 0 in this order);
  empty mask  m = 0 and every output is zero.
This is NOT pinned against cv2 itself: cv2.minAreaRect works from the same hull, so it can differ only in float rounding and in
which of several equal-area rectangles it returns."""
from fractions import Fraction

import numpy as np


def row_extents(mask) -> np.ndarray:
    """int32 [h, 3]: first set column, last set column and pixel count of every row; (-1, -1, 0) for an empty row."""
    m = np.asarray(mask) != 0
    w = m.shape[1]
    cnt = m.sum(1)
    first = np.where(cnt > 0, m.argmax(1), -1)
    last = np.where(cnt > 0, w - 1 - m[:, ::-1].argmax(1), -1)
    return np.stack([first, last, cnt], axis=1).astype(np.int32)


def _chain(pts, sign):
    """Strict vertices of the convex minorant (sign = +1) / concave majorant (sign = -1) of x over y, pts = [(x, y)] by rising y."""
    out = []
    for (x, y) in pts:
        while len(out) >= 2:
            (x1, y1), (x2, y2) = out[-2], out[-1]
            # out[-1] stays only if it lies strictly on the outer side of the segment out[-2] -> (x, y)
            cross = (x2 - x1) * (y - y1) - (x - x1) * (y2 - y1)
            if sign * cross < 0:
                break
            out.pop()
        out.append((x, y))
    return out


def hull(mask, x0: int = 0, y0: int = 0):
    """The ordered strict hull vertices [(x, y)] of the definition above (Python ints); [] for an empty mask."""
    ext = row_extents(mask)
    rows = [y for y in range(ext.shape[0]) if ext[y, 2] > 0]
    if not rows:
        return []
    left = _chain([(x0 + int(ext[y, 0]), y0 + y) for y in rows], +1)
    right = _chain([(x0 + int(ext[y, 1]), y0 + y) for y in rows], -1)[::-1]
    if right and right[0] == left[-1]:
        right = right[1:]
    if right and right[-1] == left[0]:
        right = right[:-1]
    return left + right


def hbox(mask, x0: int = 0, y0: int = 0):
    ys, xs = np.nonzero(np.asarray(mask))
    if len(xs) == 0:
        return (0, 0, 0, 0)
    return (x0 + int(xs.min()), y0 + int(ys.min()), x0 + int(xs.max()), y0 + int(ys.max()))


def candidate(verts, dx: int, dy: int):
    """(pmin, pmax, qmin, qmax) of the hull vertices along (dx, dy)."""
    ps = [x * dx + y * dy for x, y in verts]
    qs = [-x * dy + y * dx for x, y in verts]
    return min(ps), max(ps), min(qs), max(qs)


def record(verts):
    """The int64 [8] record of a vertex list, as Python ints."""
    m = len(verts)
    if m == 0:
        return (0,) * 8
    xs, ys = np.array([v[0] for v in verts], dtype=np.int64), np.array([v[1] for v in verts], dtype=np.int64)
    best = None
    for k in range(m):
        (xa, ya), (xb, yb) = verts[k], verts[(k + 1) % m]
        dx, dy = (xb - xa, yb - ya) if m > 1 else (1, 0)
        p, q = xs * dx + ys * dy, ys * dx - xs * dy                # |p|, |q| < 2^30: exact in int64
        pmin, pmax, qmin, qmax = int(p.min()), int(p.max()), int(q.min()), int(q.max())
        num, den = (pmax - pmin) * (qmax - qmin), dx * dx + dy * dy            # Python integers: the area num / den, exactly
        if best is None or num * best[0][1] < best[0][0] * den:
            best = ((num, den), (dx, dy, pmin, pmax, qmin, qmax))
    area2 = sum(verts[(k + 1) % m][0] * verts[k][1] - verts[k][0] * verts[(k + 1) % m][1] for k in range(m))
    return best[1] + (m, area2)


def corners(rec) -> np.ndarray:
    """float32 [4, 2] of a record: one fp64 division per coordinate, rounded to fp32."""
    dx, dy, pmin, pmax, qmin, qmax, m, _ = (int(v) for v in rec)
    out = np.zeros((4, 2), dtype=np.float32)
    if m == 0:
        return out
    L = dx * dx + dy * dy
    for i, (p, q) in enumerate(((pmin, qmin), (pmax, qmin), (pmax, qmax), (pmin, qmax))):
        out[i, 0] = np.float32(np.float64(p * dx - q * dy) / np.float64(L))
        out[i, 1] = np.float32(np.float64(p * dy + q * dx) / np.float64(L))
    return out


def mask_boxes(masks, x0: int = 0, y0: int = 0):
    """masks [n, h, w] -> (hbox int32 [n, 4], rbox float32 [n, 4, 2], record int64 [n, 8]), what samrs_mask_boxes writes."""
    masks = np.asarray(masks)
    n = masks.shape[0]
    hb, rb, rec = np.zeros((n, 4), np.int32), np.zeros((n, 4, 2), np.float32), np.zeros((n, 8), np.int64)
    for j in range(n):
        v = hull(masks[j], x0, y0)
        hb[j] = hbox(masks[j], x0, y0)
        rec[j] = record(v)
        rb[j] = corners(rec[j])
    return hb, rb, rec


# ---- brute force, for tests/test_mask_boxes_host.py ---------------------------------------------------------------------------
def monotone_chain_hull(points):
    """Andrew's monotone chain over all points [(x, y)]: strict vertices, counter-clockwise in (x, y)."""
    pts = sorted(set(points))
    if len(pts) <= 2:
        return pts

    def half(seq):
        out = []
        for p in seq:
            while len(out) >= 2 and (out[-1][0] - out[-2][0]) * (p[1] - out[-2][1]) - (out[-1][1] - out[-2][1]) * (p[0] - out[-2][0]) <= 0:
                out.pop()
            out.append(p)
        return out
    lower, upper = half(pts), half(pts[::-1])
    return lower[:-1] + upper[:-1]


def in_definition_order(ccw):
    """A counter-clockwise vertex list re-ordered as the definition orders it: reversed, starting at the smallest (y, x)."""
    if len(ccw) <= 1:
        return list(ccw)
    cw = list(ccw)[::-1]
    i = min(range(len(cw)), key=lambda k: (cw[k][1], cw[k][0]))
    return cw[i:] + cw[:i]


def min_area_all_pairs(points):
    """The smallest bounding-rectangle area (a Fraction) over the directions of ALL pairs of points, a superset of the hull edges."""
    pts = sorted(set(points))
    if len(pts) == 1:
        return Fraction(0)
    best = None
    seen = set()
    for i in range(len(pts)):
        for j in range(len(pts)):
            if i == j:
                continue
            dx, dy = pts[j][0] - pts[i][0], pts[j][1] - pts[i][1]
            g = int(np.gcd(dx, dy))
            key = (dx // g, dy // g)
            if key in seen or (-key[0], -key[1]) in seen:
                continue
            seen.add(key)
            pmin, pmax, qmin, qmax = candidate(pts, key[0], key[1])
            a = Fraction((pmax - pmin) * (qmax - qmin), key[0] ** 2 + key[1] ** 2)
            if best is None or a < best:
                best = a
    return best


# ---- shapes the tests and tools/mask_boxes_bench.py share ---------------------------------------------------------------------
def rotated_bar(side: int, deg: float, length: float, width: float) -> np.ndarray:
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
    c = (side - 1) / 2.0
    t = np.deg2rad(deg)
    u = (xx - c) * np.cos(t) + (yy - c) * np.sin(t)
    v = -(xx - c) * np.sin(t) + (yy - c) * np.cos(t)
    return ((np.abs(u) <= length / 2) & (np.abs(v) <= width / 2)).astype(np.uint8)


def disk(side: int, diameter: float) -> np.ndarray:
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
    c = (side - 1) / 2.0
    return (((xx - c) ** 2 + (yy - c) ** 2) <= (diameter / 2.0) ** 2).astype(np.uint8)


def diamond(side: int, r: int) -> np.ndarray:
    yy, xx = np.mgrid[0:side, 0:side]
    c = side // 2
    return ((np.abs(xx - c) + np.abs(yy - c)) <= r).astype(np.uint8)
