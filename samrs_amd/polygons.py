"""Reading the result of ``Engine.mask_polygons`` (samrs_mask_polygons) on the host: numpy only.

Vertices are corners of the pixel lattice: (x, y) is the top-left corner of pixel (row y, col x), so a ring encloses exactly the squares
of its pixels.  Outer rings have a positive signed area (clockwise on screen, y down), holes a negative one."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

Ring = Tuple[np.ndarray, bool]


def _np(t) -> np.ndarray:
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def rings_of(table, rings, vertices, j: int) -> Optional[List[Ring]]:
    """The rings of mask `j` as a list of (int32 [k, 2] vertices, is_hole), in the order the library wrote them (ascending smallest
    edge).  None when the mask was not traced or placed (a negative ring count: over the edge cap, or a full buffer)."""
    t = _np(table)[j]
    first_ring, n_rings, first_vertex = int(t[0]), int(t[1]), int(t[2])
    if n_rings < 0:
        return None
    rec = _np(rings)[first_ring:first_ring + n_rings]
    v = _np(vertices)
    out = []
    for r in rec:
        a = first_vertex + int(r[0])
        out.append((np.ascontiguousarray(v[a:a + int(r[1])], dtype=np.int32), bool(r[2] < 0)))
    return out


def hole_pixel(pts: np.ndarray) -> Tuple[int, int]:
    """(x, y) of the pixel a hole's ring record names -- the pixel that owns the ring's smallest edge --, in the vertices' frame: the
    ring's topmost lattice line carries only bottom edges, of pixels in the row above it, and the smallest of them is the leftmost.
    A set pixel of the component the hole lies in."""
    p = np.asarray(pts, np.int64)
    top = p[:, 1].min()
    return int(p[p[:, 1] == top, 0].min()), int(top) - 1


def signed_area2(pts: np.ndarray) -> int:
    """twice the signed shoelace area of a closed ring [k, 2] (positive: an outer ring of this library)"""
    p = np.asarray(pts, np.int64)
    q = np.roll(p, -1, axis=0)
    return int((p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]).sum())


def _contains(pts: np.ndarray, x2: int, y2: int) -> bool:
    """even-odd: is the point (x2 / 2, y2 / 2) -- a pixel centre, never on a lattice line -- inside the rectilinear ring"""
    p = np.asarray(pts, np.int64) * 2
    q = np.roll(p, -1, axis=0)
    vert = p[:, 0] == q[:, 0]                                      # vertical edges cross the horizontal ray to the right
    lo = np.minimum(p[:, 1], q[:, 1])
    hi = np.maximum(p[:, 1], q[:, 1])
    return bool((vert & (p[:, 0] > x2) & (lo < y2) & (y2 < hi)).sum() & 1)


def nest(rings_list: Sequence[Ring]) -> List[Tuple[np.ndarray, List[np.ndarray]]]:
    """[(outer, [holes])] from ``rings_of``, the outer rings in their order.  A hole's parent is the smallest-area outer ring that
    contains the centre of the pixel recorded in the hole's ring record (``hole_pixel`` finds the same pixel from the vertices): a set
    pixel of the component the hole lies in.  What GeoJSON / labelme writers need."""
    outers = [(r[0], []) for r in rings_list if not r[1]]
    areas = [signed_area2(o[0]) for o in outers]
    for r in rings_list:
        if not r[1]:
            continue
        x, y = hole_pixel(r[0])
        best = None
        for k, (o, _) in enumerate(outers):
            if _contains(o, 2 * x + 1, 2 * y + 1) and (best is None or areas[k] < areas[best]):
                best = k
        if best is None:
            raise ValueError("a hole lies in no outer ring: the rings are not those of one mask")
        outers[best][1].append(r[0])
    return outers


def coco_segmentation(rings_list: Sequence) -> Tuple[List[List[int]], bool]:
    """(polygons, has_holes): the OUTER rings as COCO flat [x0, y0, x1, y1, ...] lists.  COCO's polygon form cannot carry holes, so
    the holes are DROPPED here and `has_holes` says whether there were any; use the RLE form where they matter."""
    polys = [[int(c) for c in r[0].reshape(-1)] for r in rings_list if not r[1]]
    return polys, any(r[1] for r in rings_list)


def rasterize(rings_list: Sequence, h: int, w: int, origin: Sequence[int] = (0, 0)) -> np.ndarray:
    """uint8 [h, w]: the even-odd fill of the rings -- the inverse of the tracing.  Every vertical ring edge toggles the pixels to its
    right in the rows it spans."""
    d = np.zeros((h, w + 1), np.int32)
    for r in rings_list:
        p = np.asarray(r[0], np.int64) - np.asarray(origin, np.int64)
        q = np.roll(p, -1, axis=0)
        for (xa, ya), (xb, yb) in zip(p.tolist(), q.tolist()):
            if xa == xb and ya != yb:
                d[min(ya, yb):max(ya, yb), xa] += 1
    return (np.cumsum(d, axis=1)[:, :w] & 1).astype(np.uint8)


def rasterize_any(rings_list: Sequence, h: int, w: int, origin: Sequence[int] = (0, 0)) -> np.ndarray:
    """uint8 [h, w]: the even-odd fill of rings with ARBITRARY integer vertices (simplified rings: ``Engine.simplify_polygons``),
    sampled at the pixel centres.  Exact, in doubled integer coordinates: the centre of pixel (row r, col c) is (2 c + 1, 2 r + 1), the
    vertices are even, so a centre's row line never passes through a vertex.  An edge (a, b) crosses the row line Y = 2 r + 1 when
    min(ya, yb) < Y < max(ya, yb), at X = xa + (Y - ya) (xb - xa) / (yb - ya); it toggles the pixels whose centre 2 c + 1 is to the
    right of X or on it (a centre exactly on an edge counts as to its right; never the case for lattice rings).  Equals ``rasterize``
    on rectilinear rings."""
    d = np.zeros((h, w + 1), np.int32)
    o = np.asarray(origin, np.int64)
    for r in rings_list:
        p = (np.asarray(r[0], np.int64) - o) * 2
        q = np.roll(p, -1, axis=0)
        for (xa, ya), (xb, yb) in zip(p.tolist(), q.tolist()):
            if ya == yb:
                continue
            lo, hi = (ya, yb) if ya < yb else (yb, ya)
            r0, r1 = max(lo // 2, 0), min(hi // 2, h)              # rows with lo < 2 r + 1 < hi
            if r0 >= r1:
                continue
            Y = 2 * np.arange(r0, r1, dtype=np.int64) + 1
            num, den = (Y - ya) * (xb - xa), yb - ya               # X = xa + num / den; first column c with 2 c + 1 >= X:
            if den < 0:
                num, den = -num, -den
            # 2 c + 1 >= xa + num / den  <=>  c >= (den (xa - 1) + num) / (2 den): the ceiling, in integers
            c = -((-(den * (xa - 1) + num)) // (2 * den))
            c = np.clip(c, 0, w)
            np.add.at(d, (np.arange(r0, r1), c), 1)
    return (np.cumsum(d, axis=1)[:, :w] & 1).astype(np.uint8)


def pack_rings(rings_lists: Sequence) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(table int64 [n, 5], rings int32 [R, 4], vertices int32 [V, 2]) in the library's layout from one ``rings_of``-style list per
    row -- (int [k, 2] vertices, is_hole) pairs, or bare vertex arrays -- : the inverse of ``rings_of``, what
    ``Engine.fill_polygons`` takes once uploaded.  A None entry becomes a not-traced row (ring count = vertex count = -1, firsts -1).
    table[j] = (first ring, ring count, first vertex, vertex count, the vertex count again where the library keeps the traced edge
    count); a ring record = (first vertex relative to the row's, vertex count, twice the signed shoelace area, negated if it
    disagrees with is_hole so that the sign still says hole, 0 where the library keeps a pixel index).  Empty buffers have one
    unused row, so that they can be uploaded."""
    table = np.zeros((len(rings_lists), 5), np.int64)
    recs, verts = [], []
    nv = 0
    for j, rl in enumerate(rings_lists):
        if rl is None:
            table[j] = (-1, -1, -1, -1, 0)
            continue
        v0, r0 = nv, len(recs)
        for ring in rl:
            hole = None
            if isinstance(ring, tuple) and len(ring) == 2 and np.ndim(ring[0]) == 2:
                ring, hole = ring[0], bool(ring[1])
            p = np.asarray(ring, dtype=np.int64).reshape(-1, 2)
            if len(p) < 1:
                raise ValueError(f"row {j}: a ring without vertices")
            if np.abs(p).max() >= 1 << 31:
                raise ValueError(f"row {j}: a vertex does not fit int32")
            a2 = signed_area2(p)
            if hole is not None and a2 != 0 and (a2 < 0) != hole:
                a2 = -a2
            recs.append((nv - v0, len(p), int(np.clip(a2, -(1 << 31) + 1, (1 << 31) - 1)), 0))
            verts.append(p.astype(np.int32))
            nv += len(p)
        table[j] = (r0, len(recs) - r0, v0, nv - v0, nv - v0)
    rings = np.asarray(recs, dtype=np.int32).reshape(-1, 4) if recs else np.zeros((1, 4), np.int32)
    vertices = np.concatenate(verts).reshape(-1, 2) if verts else np.zeros((1, 2), np.int32)
    return table, np.ascontiguousarray(rings), np.ascontiguousarray(vertices)


def fill_device(engine, rings_lists: Sequence, h: int, w: int, origin: Sequence[int] = (0, 0)):
    """uint8 [n, h, w] tensor on the engine's device: ``rasterize_any`` of every entry of `rings_lists`, on the GPU
    (``pack_rings`` -> upload -> ``Engine.fill_polygons``).  A None entry fills as the empty mask."""
    from . import engine as _engine            # the one function here that needs a device: this module itself stays numpy only
    torch = _engine.torch
    table, rings, vertices = pack_rings(rings_lists)
    dev = engine.device
    masks, _ = engine.fill_polygons(torch.from_numpy(table).to(dev), torch.from_numpy(rings).to(dev), torch.from_numpy(vertices).to(dev),
                                    (h, w), origin, counts_out=False)
    return masks


def iou_from_counts(counts) -> np.ndarray:
    """float64 [...]: inter / (fill + ref - inter) from ``Engine.fill_polygons``'s counts [..., 3] = (fill, ref, both).  Two empty
    sides give 1.0; a row with fill = -1 (not rings: not traced, not placed) gives NaN."""
    c = np.asarray(_np(counts), dtype=np.int64)
    fill, ref, both = c[..., 0], c[..., 1], c[..., 2]
    union = fill + ref - both
    out = np.where(union > 0, both / np.maximum(union, 1).astype(np.float64), 1.0)
    return np.where(fill < 0, np.nan, out)
