"""Three references for rt_overlap_triangles_device (include/rt_api.h; DESIGN.md §5 "Triangle overlaps"), none with a tree:

 * brute32: the canonical binary32 predicate restated in numpy from the header and DESIGN text, over every (query, instance, triangle)
   pair, with the exactly rounded binary32 fma of tests/closest_reference.py behind dot3 and cross3 and np.fmin / np.fmax for fminf /
   fmaxf.  The GPU is held to it bit for bit.
 * brute64: the same seventeen axes in binary64 on the same binary32 A, B, C, P0, P1, P2, with the separation of every pair: the largest
   gap over the axes (negative: the smallest penetration), each relative to the first-order size of what binary32 rounds on that axis.
 * exact: an independently formulated rational test (fractions.Fraction) for lattice inputs: two triangles meet iff an edge of one
   meets the other closed triangle; an edge in the other's plane meets it iff it crosses one of its edges or ends inside it.  It guards
   the choice of axes, not the rounding.

Step 2 of the predicate is step 2 of the box predicate with the query's bounds as the box (tests/overlap_reference.py), exact in
binary32 and binary64 alike, so all three evaluate the rest on the pairs that survive it only."""
from fractions import Fraction

import numpy as np

from tests import overlap_reference as orf
from tests.closest_reference import F, cross3, dot3

Triangles = orf.Triangles
COLS = [0, 1, 2, 4, 5, 6, 8, 9, 10]   # the vertex components of a record (words 3, 7 and 11 are ignored)


def valid_queries(q):
    """(n,) bool: every vertex component finite"""
    return np.isfinite(np.asarray(q, F).reshape(-1, 12)[:, COLS]).all(-1)


def bounds(q):
    """the (n, 8) box records of the queries' bounds (fminf / fmaxf of the vertices); an invalid query gives an invalid box"""
    q = np.asarray(q, F).reshape(-1, 12)
    P = q[:, COLS].reshape(-1, 3, 3)
    b = np.zeros((len(q), 8), F)
    b[:, 0:3] = np.fmin(np.fmin(P[:, 0], P[:, 1]), P[:, 2])
    b[:, 4:7] = np.fmax(np.fmax(P[:, 0], P[:, 1]), P[:, 2])
    b[~valid_queries(q), 0] = np.nan
    return b


def surviving_pairs(tris, q, cull_mask=0xFF):
    """(query index, triangle index) arrays of the pairs of valid queries and finite triangles of admitted instances that step 2 does not
    separate, in (query, inst, prim) order"""
    return orf.surviving_pairs(tris, bounds(q), cull_mask)


def _axes(P0, P1, P2, A, B, C, f32):
    """steps 3 to 7 on pair arrays (3, m): yields (q1, q2, ta, tb, tc, norm, degree) per axis: the projections of p1 and p2 (the query's
    third is 0) and of a, b, c, the 1-norm of the axis and how many edges it is a product of.  f32: binary32 with the canonical
    operations; else binary64."""
    if f32:
        dot, cross = dot3, cross3
    else:
        P0, P1, P2, A, B, C = (x.astype(np.float64) for x in (P0, P1, P2, A, B, C))
        dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]   # noqa: E731
        cross = lambda a, b: (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])   # noqa: E731
    p1, p2 = tuple(P1 - P0), tuple(P2 - P0)
    a, b, c = tuple(A - P0), tuple(B - P0), tuple(C - P0)
    sub = lambda x, y: tuple(x[k] - y[k] for k in range(3))   # noqa: E731
    g = [p1, sub(p2, p1), p2]
    f = [sub(b, a), sub(c, b), sub(a, c)]
    n, m = cross(g[0], g[2]), cross(f[0], f[1])
    axes = [(n, 2), (m, 2)] + [(cross(gi, fj), 2) for gi in g for fj in f] + [(cross(n, gi), 3) for gi in g] + [(cross(m, fj), 3) for fj in f]
    for L, degree in axes:
        yield dot(L, p1), dot(L, p2), dot(L, a), dot(L, b), dot(L, c), np.abs(L[0]) + np.abs(L[1]) + np.abs(L[2]), degree


def _pair_arrays(tris, q, qi, ti):
    q = np.asarray(q, F).reshape(-1, 12)
    return q[qi, 0:3].T, q[qi, 4:7].T, q[qi, 8:11].T, tris.A[ti].T, tris.B[ti].T, tris.C[ti].T


def candidates32(tris, q, qi, ti):
    """(pairs,) bool: the canonical predicate does not separate the pair (steps 3 to 7; step 2 is surviving_pairs')"""
    sep = np.zeros(len(qi), bool)
    zero = F(0)
    with np.errstate(all="ignore"):
        for q1, q2, ta, tb, tc, _, _ in _axes(*_pair_arrays(tris, q, qi, ti), f32=True):
            qmin, qmax = np.fmin(np.fmin(zero, q1), q2), np.fmax(np.fmax(zero, q1), q2)
            tmin, tmax = np.fmin(np.fmin(ta, tb), tc), np.fmax(np.fmax(ta, tb), tc)
            sep |= (qmin > tmax) | (qmax < tmin)
    return ~sep


def separation64(tris, q, qi, ti):
    """(pairs,) float64: the largest gap over the twenty axes (step 2's three included), each relative to the magnitudes involved, as
    overlap_reference.separation64 defines it for boxes: > 0 separated by that much, <= 0 not separated, penetrating by that much.  With
    M the largest coordinate of the pair, V the largest centred coordinate, E the largest edge component and |L|_1 the 1-norm of the
    axis: a bounds axis compares coordinates (scale M).  A projection dot3(L, v) rounds at |L|_1 V and carries the rounding of L times V;
    L is a product of two edges (n, m, the nine crosses) or three (the in-plane axes), each edge a difference of centred coordinates
    that are themselves rounded at V: the rounding of L has the size E V, or E E V (scale |L|_1 V + E^(d-2) E V V with d edges).  An axis
    of zero norm (zero-area triangles, parallel edges) separates nothing."""
    P0, P1, P2, A, B, C = (x.astype(np.float64) for x in _pair_arrays(tris, q, qi, ti))
    M = np.max([np.abs(x).max(0) for x in (P0, P1, P2, A, B, C)], axis=0)
    M = np.where(M > 0, M, 1.0)
    V = np.max([np.abs(x - P0).max(0) for x in (P1, P2, A, B, C)], axis=0)
    E = np.max([np.abs(x).max(0) for x in (P1 - P0, P2 - P1, P2 - P0, B - A, C - B, A - C)], axis=0)
    s = np.full(len(qi), -np.inf)
    for k in range(3):
        tmn, tmx = np.minimum(np.minimum(A[k], B[k]), C[k]), np.maximum(np.maximum(A[k], B[k]), C[k])
        qmn, qmx = np.minimum(np.minimum(P0[k], P1[k]), P2[k]), np.maximum(np.maximum(P0[k], P1[k]), P2[k])
        s = np.maximum(s, np.maximum(tmn - qmx, qmn - tmx) / M)
    with np.errstate(all="ignore"):
        for q1, q2, ta, tb, tc, norm, degree in _axes(P0, P1, P2, A, B, C, f32=False):
            qmin, qmax = np.minimum(np.minimum(0.0, q1), q2), np.maximum(np.maximum(0.0, q1), q2)
            tmin, tmax = np.minimum(np.minimum(ta, tb), tc), np.maximum(np.maximum(ta, tb), tc)
            gap = np.maximum(qmin - tmax, tmin - qmax)
            scale = norm * V + (E * V * V if degree == 2 else E * E * V * V)
            s = np.maximum(s, np.where(norm > 0, gap / np.where(scale > 0, scale, 1.0), -np.inf))
    return s


def brute32(scene, q, cull_mask=0xFF, max_ids=16, tris=None):
    """counts (n,) uint32 and ids (n, max_ids, 2) int32 of the canonical binary32 predicate over all (query, instance, triangle) pairs"""
    tris = tris or Triangles(scene)
    n = len(np.asarray(q, F).reshape(-1, 12))
    qi, ti = surviving_pairs(tris, q, cull_mask)
    return orf.rows(scene, n, qi, ti, candidates32(tris, q, qi, ti), max_ids)


def brute64(scene, q, cull_mask=0xFF, max_ids=16, tris=None):
    """the same in binary64 on the same binary32 inputs (a pair is a candidate when its separation is <= 0)"""
    tris = tris or Triangles(scene)
    n = len(np.asarray(q, F).reshape(-1, 12))
    qi, ti = surviving_pairs(tris, q, cull_mask)
    return orf.rows(scene, n, qi, ti, separation64(tris, q, qi, ti) <= 0, max_ids)


# ---- the rational test ----------------------------------------------------------------------------------------------------------

def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _in_triangle(x, T, N):
    """x, a point of the plane of the non-degenerate triangle T with normal N, lies in the closed triangle"""
    u, v, w = T
    return _dot(N, _cross(_sub(v, u), _sub(x, u))) >= 0 and _dot(N, _cross(_sub(w, v), _sub(x, v))) >= 0 and _dot(N, _cross(_sub(u, w), _sub(x, w))) >= 0


def _segments_meet(s, t, p, q, N):
    """the closed segments st and pq of one plane with normal N have a common point"""
    o = lambda a, b, c: _dot(N, _cross(_sub(b, a), _sub(c, a)))   # noqa: E731
    between = lambda a, b, c: _dot(_sub(c, a), _sub(c, b)) <= 0   # noqa: E731  (c, collinear with ab, lies on the closed segment)
    o1, o2, o3, o4 = o(s, t, p), o(s, t, q), o(p, q, s), o(p, q, t)
    if o1 * o2 < 0 and o3 * o4 < 0:
        return True
    return (o1 == 0 and between(s, t, p)) or (o2 == 0 and between(s, t, q)) or (o3 == 0 and between(p, q, s)) or (o4 == 0 and between(p, q, t))


def _segment_meets_triangle(s, t, T):
    u, v, w = T
    N = _cross(_sub(v, u), _sub(w, u))
    ds, dt = _dot(N, _sub(s, u)), _dot(N, _sub(t, u))
    if (ds > 0 and dt > 0) or (ds < 0 and dt < 0):
        return False
    if ds == 0 and dt == 0:   # in the plane: an end inside, or a crossing with an edge
        return _in_triangle(s, T, N) or _in_triangle(t, T, N) or any(_segments_meet(s, t, a, b, N) for a, b in ((u, v), (v, w), (w, u)))
    k = Fraction(ds) / Fraction(ds - dt)
    x = tuple(s[i] + k * (t[i] - s[i]) for i in range(3))
    return _in_triangle(x, T, N)


def exact_pair(T1, T2):
    """two non-degenerate triangles with rational vertices have a common point"""
    e = lambda T: ((T[0], T[1]), (T[1], T[2]), (T[2], T[0]))   # noqa: E731
    return any(_segment_meets_triangle(s, t, T2) for s, t in e(T1)) or any(_segment_meets_triangle(s, t, T1) for s, t in e(T2))


def exact(tris, q, qi, ti):
    """(pairs,) bool: exact_pair of the pairs (the binary32 vertices taken as the rationals they are); every triangle non-degenerate"""
    q = np.asarray(q, F).reshape(-1, 12)
    rat = lambda v: tuple(Fraction(float(x)) for x in v)   # noqa: E731
    out = np.zeros(len(qi), bool)
    for j, (i, t) in enumerate(zip(qi, ti)):
        T1 = (rat(q[i, 0:3]), rat(q[i, 4:7]), rat(q[i, 8:11]))
        T2 = (rat(tris.A[t]), rat(tris.B[t]), rat(tris.C[t]))
        out[j] = exact_pair(T1, T2)
    return out
