"""The host statement of samrs_simplify_polygons (include/samrs_hip.h states the rule): a plain recursion over Python ints, the
sequential statement of what the call changes in the four buffers, and a checker that is independent of both."""
import sys

import numpy as np

EPS_Q_MAX = 16384


def _sub(p, a):
    return p[0] - a[0], p[1] - a[1]


def _cross(u, v):
    return u[0] * v[1] - u[1] * v[0]


def _dot(u, v):
    return u[0] * v[0] + u[1] * v[1]


def dist_nd(a, b, p):
    """(N, D): the squared distance of p to the SEGMENT a b is N / D, in integers"""
    ab, ap = _sub(b, a), _sub(p, a)
    L = _dot(ab, ab)
    if L == 0:
        return _dot(ap, ap), 1
    t = _dot(ap, ab)
    if t <= 0:
        return _dot(ap, ap) * L, L
    if t >= L:
        bp = _sub(p, b)
        return _dot(bp, bp) * L, L
    c = _cross(ab, ap)
    return c * c, L


def anchors(v):
    """(A, B, C) of a ring given as a list of (x, y) Python ints: ties to the smallest index"""
    k = len(v)
    a = v[0]
    B = max(range(k), key=lambda i: (_dot(_sub(v[i], a), _sub(v[i], a)), -i))
    ab = _sub(v[B], a)
    C = max(range(k), key=lambda i: (abs(_cross(ab, _sub(v[i], a))), -i))
    return 0, B, C


def simplify_ring(pts, eps_q):
    """(sorted kept indices, recursion depth reached) of one closed ring [k, 2].  The three chains between the anchors are depth 1; a
    chain that keeps a vertex calls its two halves one level deeper."""
    assert 1 <= eps_q <= EPS_Q_MAX
    v = [(int(x), int(y)) for x, y in np.asarray(pts).tolist()]
    k = len(v)
    if k <= 3:
        return list(range(k)), 0
    kept = set(anchors(v))
    eps2 = eps_q * eps_q
    deepest = [0]

    def chain(i, j, depth):                                        # j == k stands for index 0 again
        deepest[0] = max(deepest[0], depth)
        a, b = v[i], v[j % k]
        best, arg, D = -1, -1, 1
        for m in range(i + 1, j):
            N, D = dist_nd(a, b, v[m])
            if N > best:
                best, arg = N, m
        if arg < 0 or not best > (eps2 * D) // 256:
            return
        kept.add(arg)
        chain(i, arg, depth + 1)
        chain(arg, j, depth + 1)

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, k + 200))
    try:
        s = sorted(kept)
        for i, j in zip(s, s[1:] + [k]):
            chain(i, j, 1)
    finally:
        sys.setrecursionlimit(old)
    return sorted(kept), deepest[0]


def simplify_ring_fast(pts, eps_q):
    """The kept indices of ``simplify_ring``, with each chain's N evaluated as one numpy int64 expression (exact within the limits
    of samrs_mask_boxes: every product is below 2^62) and an explicit stack: for the pipelines' masks, whose rings run to tens of
    thousands of vertices.  tests/test_polygon_simplify_host.py holds it against the plain recursion."""
    v = np.asarray(pts, np.int64)
    k = len(v)
    if k <= 24:
        return simplify_ring(pts, eps_q)[0]
    d = v - v[0]
    B = int(np.argmax((d * d).sum(1)))                              # argmax: the first of equal maxima
    C = int(np.argmax(np.abs(d[B, 0] * d[:, 1] - d[B, 1] * d[:, 0])))
    kept = {0, B, C}
    eps2 = eps_q * eps_q
    s = sorted(kept)
    stack = list(zip(s, s[1:] + [k]))
    while stack:
        i, j = stack.pop()
        if j - i < 2:
            continue
        a, b, p = v[i], v[j % k], v[i + 1:j]
        ab, ap = b - a, p - a
        L = int(ab @ ab)
        pa = (ap * ap).sum(1)
        if L == 0:
            N, D = pa, 1
        else:
            t = ap @ ab
            bp = p - b
            c = ab[0] * ap[:, 1] - ab[1] * ap[:, 0]
            N, D = np.where(t <= 0, pa * L, np.where(t >= L, (bp * bp).sum(1) * L, c * c)), L
        m = int(np.argmax(N))
        if int(N[m]) > (eps2 * D) // 256:
            kept.add(i + 1 + m)
            stack += [(i, i + 1 + m), (i + 1 + m, j)]
    return sorted(kept)


def row_placed(t):
    return all(int(x) >= 0 for x in t[:4])


def simplify_buffers(table, rings, vertices, cursor, eps_q, fast=False):
    """What samrs_simplify_polygons leaves in (table, rings, vertices, cursor), from numpy copies of what the samrs_mask_polygons
    calls wrote; also the deepest recursion over all rings.  Vertices at and behind the new end keep their old content."""
    t, r, v, c = (np.array(x, copy=True) for x in (table, rings, vertices, cursor))
    t0, r0, v0 = np.asarray(table), np.asarray(rings), np.asarray(vertices)
    placed = [j for j in range(len(t0)) if row_placed(t0[j])]
    depth = 0
    if not placed:
        return t, r, v, c, depth
    pos = int(t0[placed[0], 2])
    for j in placed:
        fr, nr, fv = int(t0[j, 0]), int(t0[j, 1]), int(t0[j, 2])
        first = pos
        for q in range(fr, fr + nr):
            a, k = fv + int(r0[q, 0]), int(r0[q, 1])
            idx, d = (simplify_ring_fast(v0[a:a + k], eps_q), 0) if fast else simplify_ring(v0[a:a + k], eps_q)
            depth = max(depth, d)
            v[pos:pos + len(idx)] = v0[a:a + k][idx]
            r[q, 0], r[q, 1] = pos - first, len(idx)
            pos += len(idx)
        t[j, 2], t[j, 3] = first, pos - first
    c[0] = pos
    return t, r, v, c, depth


def check_ring(orig, simp, eps_q):
    """The three properties, in integers: `simp` is a subsequence of `orig` that begins with orig[0]; it has at least 3 vertices;
    every original vertex lies within eps_q / 16 of the chord segment that replaced it (256 N <= eps_q^2 D)."""
    o = [(int(x), int(y)) for x, y in np.asarray(orig).tolist()]
    s = [(int(x), int(y)) for x, y in np.asarray(simp).tolist()]
    assert len(s) >= 3 and s[0] == o[0], (len(s), s[:1], o[:1])
    at, where = 0, []
    for p in s:                                                    # greedy subsequence match: positions in the original
        while at < len(o) and o[at] != p:
            at += 1
        assert at < len(o), "not a subsequence of the original ring"
        where.append(at)
        at += 1
    eps2 = eps_q * eps_q
    k = len(o)
    for i, j in zip(where, where[1:] + [k]):
        a, b = o[i], o[j % k]
        for m in range(i + 1, j):
            N, D = dist_nd(a, b, o[m])
            if 256 * N > eps2 * D:                                 # the greedy match may sit on an earlier visit of a repeated point
                return check_ring_indices(o, s, eps2)
    return True


def check_ring_indices(o, s, eps2):
    """the same with every possible match of a repeated lattice point tried (rings that touch themselves at a saddle vertex)"""
    k = len(o)

    def ok(i, j):
        a, b = o[i], o[j % k]
        return all(256 * dist_nd(a, b, o[m])[0] <= eps2 * dist_nd(a, b, o[m])[1] for m in range(i + 1, j))

    reach = {0}                                                    # positions of s[n] whose prefix chains all pass
    for n in range(1, len(s)):
        nxt = set()
        for i in reach:
            for j in range(i + 1, k):
                if o[j] == s[n] and ok(i, j):
                    nxt.add(j)
        reach = nxt
        assert reach, f"vertex {n} of the simplified ring: no placement within the tolerance"
    assert any(ok(i, k) for i in reach), "the closing chain leaves the tolerance"
    return True
