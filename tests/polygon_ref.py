"""Host restatement of samrs_mask_polygons (include/samrs_hip.h): the crack edges of a mask enumerated with numpy, their successor
by the three-way rule, and a plain sequential walk along it.  No GPU, no cv2, no oracle.  The device must match every stage exactly.

Lattice: vertex (x, y) is the top-left corner of pixel (row y, col x).  Edge id = 4 * (y * w + x) + d of a set pixel: d = 0 top
heading E, 1 right heading S, 2 bottom heading W, 3 left heading N -- the set pixel on the right hand of travel, y down."""
import numpy as np

DX = np.array([1, 0, -1, 0])
DY = np.array([0, 1, 0, -1])
# start vertex of edge d relative to the pixel's top-left corner
SX = np.array([0, 1, 1, 0])
SY = np.array([0, 0, 1, 1])


def _padded(mask):
    m = np.asarray(mask) != 0
    p = np.zeros((m.shape[0] + 4, m.shape[1] + 4), bool)
    p[2:-2, 2:-2] = m
    return p


def edges(mask):
    """(ids int64 ascending, succ = compact index of each edge's successor, corner uint8) of one mask [h, w]."""
    h, w = mask.shape
    p = _padded(mask)
    ys, xs = np.nonzero(p[2:-2, 2:-2])
    ids = []
    for d in range(4):
        out = (d + 3) % 4                                      # the outward normal of edge d
        has = ~p[ys + 2 + DY[out], xs + 2 + DX[out]]
        ids.append(4 * (ys[has].astype(np.int64) * w + xs[has]) + d)
    ids = np.sort(np.concatenate(ids)) if ids else np.zeros(0, np.int64)
    d = (ids & 3).astype(np.int64)
    pix = ids >> 2
    y, x = pix // w, pix % w
    dl = (d + 3) % 4
    lx, ly = x + DX[d] + DX[dl], y + DY[d] + DY[dl]            # L: ahead on the left
    rx, ry = x + DX[d], y + DY[d]                              # R: straight ahead
    Lset = p[ly + 2, lx + 2]
    Rset = p[ry + 2, rx + 2]
    sx = np.where(Lset, lx, np.where(Rset, rx, x))
    sy = np.where(Lset, ly, np.where(Rset, ry, y))
    sd = np.where(Lset, dl, np.where(Rset, d, (d + 1) % 4))
    sid = 4 * (sy * w + sx) + sd
    succ = np.searchsorted(ids, sid)
    assert ids.size == 0 or (succ < ids.size).all() and (ids[succ] == sid).all(), "a successor is not an edge"
    # the predecessor runs straight into an edge iff the pixel behind is set and the pixel behind on the left is not
    bx, by = x - DX[d], y - DY[d]
    straight = p[by + 2, bx + 2] & ~p[by + DY[dl] + 2, bx + DX[dl] + 2]
    return ids, succ.astype(np.int64), (~straight).astype(np.uint8)


def walk(ids, succ):
    """(leader, rank) per edge by a sequential walk: leader = compact index of the smallest edge of the ring, rank = distance from it."""
    n = ids.size
    leader = np.full(n, -1, np.int64)
    rank = np.zeros(n, np.int64)
    s = succ.tolist()
    lead, rk = leader.tolist(), rank.tolist()
    for i in range(n):
        if lead[i] >= 0:
            continue
        j, r = i, 0
        while lead[j] < 0:
            lead[j] = i
            rk[j] = r
            j = s[j]
            r += 1
        assert j == i, "the successor is not a bijection"
    return np.array(lead, np.int64), np.array(rk, np.int64)


def trace(mask, x0=0, y0=0):
    """One mask -> (vertices int32 [k, 2], rings int32 [r, 4], edge count); rings as the C ABI states them."""
    h, w = mask.shape
    ids, succ, corner = edges(mask)
    n = ids.size
    if n == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0, 4), np.int32), 0
    leader, rank = walk(ids, succ)
    order = np.lexsort((rank, leader))                         # rings by leader, edges by rank
    d = ids & 3
    pix = ids >> 2
    vx = pix % w + SX[d]
    vy = pix // w + SY[d]
    ex = vx + DX[d]
    ey = vy + DY[d]
    term = vx * ey - ex * vy
    verts, rings = [], []
    lo = leader[order]
    starts = np.flatnonzero(np.r_[True, lo[1:] != lo[:-1]])
    ends = np.r_[starts[1:], n]
    for a, b in zip(starts, ends):
        e = order[a:b]
        c = e[corner[e] != 0]
        rings.append((len(verts), c.size, int(term[e].sum()), int(pix[e[0]])))
        verts.extend(zip((vx[c] + x0).tolist(), (vy[c] + y0).tolist()))
    return np.array(verts, np.int32).reshape(-1, 2), np.array(rings, np.int32).reshape(-1, 4), n


def mask_polygons(masks, x0=0, y0=0, max_edges=65536, vertex_capacity=1 << 40, ring_capacity=1 << 40, cursor=(0, 0)):
    """The whole call: (vertices int32 [V, 2] used part, rings int32 [R, 4] used part, cursor (vertex, ring), table int64 [n, 5]),
    the buffers starting at index 0 (entries before the incoming cursor are zero)."""
    vf, rf = int(cursor[0]), int(cursor[1])
    V = [np.zeros((vf, 2), np.int32)]
    R = [np.zeros((rf, 4), np.int32)]
    table = np.zeros((len(masks), 5), np.int64)
    for j, m in enumerate(masks):
        ne = count_edges(m)
        if ne > max_edges:
            table[j] = (-1, -1, -1, -1, ne)
            continue
        v, r, _ = trace(m, x0, y0)
        if vf + len(v) <= vertex_capacity and rf + len(r) <= ring_capacity:
            table[j] = (rf, len(r), vf, len(v), ne)
            V.append(v)
            R.append(r)
            vf += len(v)
            rf += len(r)
        else:
            table[j] = (-1, -1 - len(r), -1, -1 - len(v), ne)
    return np.concatenate(V), np.concatenate(R), (vf, rf), table


def count_edges(mask):
    p = _padded(mask)
    c = p[2:-2, 2:-2]
    return int((c & ~p[1:-3, 2:-2]).sum() + (c & ~p[3:-1, 2:-2]).sum() + (c & ~p[2:-2, 1:-3]).sum() + (c & ~p[2:-2, 3:-1]).sum())


# ---- independent counts for the invariants ----------------------------------------------------------------------------------
def components(binary, conn8):
    """number of connected components of the True pixels (plain flood fill)"""
    b = np.asarray(binary, bool)
    h, w = b.shape
    seen = np.zeros_like(b)
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if conn8 else [])
    count = 0
    for y0, x0 in zip(*np.nonzero(b)):
        if seen[y0, x0]:
            continue
        count += 1
        stack = [(int(y0), int(x0))]
        seen[y0, x0] = True
        while stack:
            y, x = stack.pop()
            for dy, dx in nb:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and b[yy, xx] and not seen[yy, xx]:
                    seen[yy, xx] = True
                    stack.append((yy, xx))
    return count


def enclosed_background_components(mask):
    """4-connected components of the unset pixels that do not touch the outside"""
    m = np.asarray(mask) != 0
    bg = np.ones((m.shape[0] + 2, m.shape[1] + 2), bool)
    bg[1:-1, 1:-1] = ~m
    return components(bg, False) - 1                           # the padded border is one component: the outside


# ---- constructed masks ----------------------------------------------------------------------------------------------------------
def spiral(n):
    """a one-pixel-wide square spiral on an n x n canvas, inwards from the top-left corner: one ring carries every edge"""
    m = np.zeros((n, n), np.uint8)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = 1

    def free(xx, yy):
        return 0 <= xx < n and 0 <= yy < n and not m[yy, xx]

    while True:
        moved = False
        # forward while the next pixel is free and the one behind it is not a lane drawn earlier
        while free(x + dx, y + dy) and (free(x + 2 * dx, y + 2 * dy) or not (0 <= x + 2 * dx < n and 0 <= y + 2 * dy < n)):
            x, y = x + dx, y + dy
            m[y, x] = 1
            moved = True
        if not moved:
            return m
        dx, dy = -dy, dx


def ellipse(n, ax, ay, cx=None, cy=None):
    cx = n / 2 if cx is None else cx
    cy = n / 2 if cy is None else cy
    yy, xx = np.mgrid[0:n, 0:n]
    return ((((xx - cx) / ax) ** 2 + ((yy - cy) / ay) ** 2) <= 1.0).astype(np.uint8)
