"""Three references for rt_closest_triangle_device (include/rt_api.h; DESIGN.md §5 "Closest points of triangles"), none with a tree:

 * brute32: the canonical binary32 feature sequence and the key (d2, inst, prim) restated in numpy from the header and DESIGN text, over
   every triangle of every admitted instance, with the exactly rounded binary32 fma, the Scene class, the closest-point sequence and the
   side words of tests/closest_reference.py and the clamp of tests/segment_reference.py.  The GPU is held to it byte for byte.
 * brute64: deliberately NOT the feature list: the minimum, over the six edge-against-triangle pairs (the query's three edges against
   the scene triangle, the scene triangle's three edges against the query), of the binary64 distance of a segment to a triangle as a
   convex set, minimised over the segment's parameter by segment_reference's ternary search, on the same binary32 inputs.  (Two
   triangles that do not cut each other are nearest at a vertex-face or an edge-edge pair, both of which lie on an edge of one; two
   that cut each other have an edge of one through the other.)
 * altproj64: a guard of that decomposition: alternating binary64 projections, query triangle <-> scene triangle, from the centroid.
   Its result is the distance of a real point pair, hence an upper bound; where the nearest pair is unique it converges to it.

candidate_pairs() is a conservative pre-filter for brute64 (binary64 lower and upper bounds with margins): it only drops pairs that
can be neither the nearest nor a runner-up within the identity rule's reach."""
import numpy as np

from tests import closest_reference as cr
from tests.closest_reference import F, cross3, dot3
from tests.segment_reference import clamp
from vulkan_raytracing_amd.api import HIT_DTYPE

Q_EDGES = ((0, 1), (1, 2), (2, 0))      # the query's edges, in the orientation of the contract
S_EDGES = ((0, 1), (0, 2), (1, 2))      # the scene triangle's edges (a, b), (a, c), (b, c)


def valid_triangles(tris):
    """(n,) bool: finite vertices and r_max >= 0 (a NaN r_max fails)"""
    t = np.asarray(tris, F).reshape(-1, 12)
    with np.errstate(invalid="ignore"):
        return np.isfinite(t[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]).all(axis=1) & (t[:, 3] >= 0)


# ---- binary32: the canonical sequence -------------------------------------------------------------------------------------------

def _take(state, d2, uu, vv, qu, qv, allow):
    """a later feature replaces an earlier one only when its d2 is strictly smaller; a NaN d2 is skipped"""
    best = state[0]
    with np.errstate(invalid="ignore"):
        m = allow & ~np.isnan(d2) & ~(d2 >= best)
    return tuple(np.where(m, new, old) for new, old in zip((d2, uu, vv, qu, qv), state))


def _sub(p, q):
    return tuple(p[k] - q[k] for k in range(3))


def _add(p, q):
    return tuple(p[k] + q[k] for k in range(3))


def _crossing(pi, pj, a, ab, ac):
    """feature 3 of the segment query for the segment pi..pj against the plane of (a, ab, ac): (d2, u, v, s, exists)"""
    n = cross3(ab, ac)
    h0, h1 = dot3(n, _sub(pi, a)), dot3(n, _sub(pj, a))
    exists = ((h0 < 0) & (h1 > 0)) | ((h0 > 0) & (h1 < 0))
    s = clamp(h0 / (h0 - h1))
    d = _sub(pj, pi)
    X = tuple(pi[k] + s * d[k] for k in range(3))
    d2, u, v = cr.tri_d2(X, a, ab, ac)
    return d2, u, v, s, exists


def _edge_pair(pi, d, A, q, e):
    """feature 4 of the segment query for the segment pi + s d against the edge q + t e: (d2, s, t)"""
    r = _sub(pi, q)
    E, Fq, C, B = dot3(e, e), dot3(e, r), dot3(d, r), dot3(d, e)
    denom = A * E - B * B
    sg = np.where(denom != 0, clamp((B * Fq - C * E) / denom), F(0)).astype(F)
    tg = (B * sg + Fq) / E
    lo, hi = tg < 0, tg > 1
    sg = np.where(lo, clamp(-C / A), np.where(hi, clamp((B - C) / A), sg))
    tg = np.where(lo, F(0), np.where(hi, F(1), tg))
    a0, e0 = A == 0, E == 0
    ss = np.where(a0, F(0), np.where(e0, clamp(-C / A), sg)).astype(F)
    tt = np.where(a0 & e0, F(0), np.where(a0, clamp(Fq / E), np.where(e0, F(0), tg))).astype(F)
    w = tuple((pi[k] + ss * d[k]) - (q[k] + tt * e[k]) for k in range(3))
    return dot3(w, w), ss, tt


def tri_tri32(P, a, ab, ac, steps=5):
    """the canonical (d2, u, v, qu, qv) of query triangles P = (P0, P1, P2) against scene triangles (a, ab, ac): tuples of three
    broadcastable float32 arrays.  d2 is NaN where no feature has a value.  steps: how many steps of the sequence run (3: the part the
    three edge records of the segment query share)."""
    with np.errstate(all="ignore"):
        P0, P1, P2 = P
        shape = np.broadcast(P0[0], a[0]).shape
        point = np.broadcast_to(np.logical_and.reduce([(P0[k] == P1[k]) & (P0[k] == P2[k]) for k in range(3)]), shape)
        every = np.ones(shape, bool)
        zero, one = np.zeros(shape, F), np.ones(shape, F)
        state = (np.full(shape, np.nan, F), zero, zero, zero, zero)
        # 1: the query's vertices on the scene triangle
        for k, (qu, qv) in enumerate(((zero, zero), (one, zero), (zero, one))):
            d2, u, v = cr.tri_d2(P[k], a, ab, ac)
            state = _take(state, d2, u, v, qu, qv, every if k == 0 else ~point)
        # 2: the query's edges crossing the scene triangle's plane
        for k, (i, j) in enumerate(Q_EDGES):
            d2, u, v, s, exists = _crossing(P[i], P[j], a, ab, ac)
            qu, qv = ((s, zero), (F(1) - s, s), (zero, F(1) - s))[k]
            state = _take(state, d2, u, v, qu, qv, exists & ~point)
        # 3: the nine edge pairs, query-edge-major
        b = _add(a, ab)
        bc = _sub(ac, ab)
        for k, (i, j) in enumerate(Q_EDGES):
            d = _sub(P[j], P[i])
            A = dot3(d, d)
            for which, (q, e) in enumerate(((a, ab), (a, ac), (b, bc))):
                d2, ss, tt = _edge_pair(P[i], d, A, q, e)
                uu = tt if which == 0 else (zero if which == 1 else F(1) - tt)
                vv = zero if which == 0 else tt
                qu, qv = ((ss, zero), (F(1) - ss, ss), (zero, F(1) - ss))[k]
                state = _take(state, d2, uu, vv, qu, qv, ~point)
        if steps >= 5:
            # 4: the scene's vertices on the query triangle
            c = _add(a, ac)
            g0, g2 = _sub(P1, P0), _sub(P2, P0)
            V = (a, b, c)
            for k, (uu, vv) in enumerate(((zero, zero), (one, zero), (zero, one))):
                d2, qu, qv = cr.tri_d2(V[k], P0, g0, g2)
                state = _take(state, d2, uu, vv, clamp(qu), clamp(qv), ~point)
            # 5: the scene's edges crossing the query's plane
            for k, (i, j) in enumerate(S_EDGES):
                d2, qu, qv, s, exists = _crossing(V[i], V[j], P0, g0, g2)
                uu, vv = ((s, zero), (zero, s), (F(1) - s, s))[k]
                state = _take(state, d2, uu, vv, clamp(qu), clamp(qv), exists & ~point)
        return tuple(np.asarray(np.broadcast_to(x, shape), F) for x in state)


def brute32(scene, tris, cull_mask=0xFF, chunk=1 << 18, steps=5):
    """(HIT_DTYPE records, (n, 2) float32 (qu, qv), d2 float32): the smallest key (d2, inst, prim) over the admitted triangles whose d2
    is not NaN and is <= r_max * r_max, t = sqrt(d2); the miss record (t = r_max as given, params 0, d2 NaN) otherwise and for invalid
    records"""
    tr = np.ascontiguousarray(tris, F).reshape(-1, 12)
    n = len(tr)
    out = np.zeros(n, HIT_DTYPE)
    out["t"] = tr[:, 3]; out["prim"] = -1; out["inst"] = -1
    quv = np.zeros((n, 2), F)
    d2_out = np.full(n, np.nan, F)
    with np.errstate(all="ignore"):
        r2 = tr[:, 3] * tr[:, 3]
    tri = np.nonzero(scene.admitted(cull_mask))[0]
    idx = np.nonzero(valid_triangles(tr))[0]
    if len(tri) == 0:
        return out, quv, d2_out
    per = max(1, chunk // len(tri))
    ta, tab, tac = (tuple(getattr(scene, name)[tri, k][None, :] for k in range(3)) for name in ("a", "ab", "ac"))
    for k0 in range(0, len(idx), per):
        i = idx[k0:k0 + per]
        P = tuple(tuple(tr[i, 4 * v + k][:, None] for k in range(3)) for v in range(3))
        d2, u, v, qu, qv = tri_tri32(P, ta, tab, tac, steps)
        with np.errstate(invalid="ignore"):
            ok = ~np.isnan(d2) & (d2 <= r2[i][:, None])
        j = np.argmin(np.where(ok, d2, np.inf), axis=1)   # (triangles are in (inst, prim) order: the first minimum has the smallest key)
        rows = np.arange(len(i))
        j = np.where(ok[rows, j], j, np.argmax(ok, axis=1))   # (d2 = +inf within an infinite radius)
        got = ok[rows, j]
        ii, jj, rr = i[got], j[got], rows[got]
        with np.errstate(all="ignore"):
            out["t"][ii] = np.sqrt(d2[rr, jj])
        out["u"][ii] = u[rr, jj]; out["v"][ii] = v[rr, jj]
        out["prim"][ii] = scene.prim[tri[jj]]; out["inst"][ii] = scene.inst[tri[jj]]
        quv[ii, 0] = qu[rr, jj]; quv[ii, 1] = qv[rr, jj]
        d2_out[ii] = d2[rr, jj]
    return out, quv, d2_out


def edge_records(tris):
    """the three (n, 8) segment records (Pi, r_max, Pj, 0) of the query's edges, in the orientation of the contract"""
    tr = np.asarray(tris, F).reshape(-1, 12)
    out = []
    for i, j in Q_EDGES:
        s = np.zeros((len(tr), 8), F)
        s[:, 0:3] = tr[:, 4 * i:4 * i + 3]; s[:, 3] = tr[:, 3]; s[:, 4:7] = tr[:, 4 * j:4 * j + 3]
        out.append(s)
    return out


def query_points(tris, quv):
    """(n, 4) float32 point records (P0 + qu g0) + qv g2, g0 = P1 - P0, g2 = P2 - P0 (per component), with the records' r_max"""
    tr = np.asarray(tris, F).reshape(-1, 12)
    q = np.asarray(quv, F).reshape(-1, 2)
    with np.errstate(all="ignore"):
        p = (tr[:, 0:3] + q[:, 0:1] * (tr[:, 4:7] - tr[:, 0:3])) + q[:, 1:2] * (tr[:, 8:11] - tr[:, 0:3])
    return np.concatenate([p, tr[:, 3:4]], axis=1).astype(F)


def side_words(scene, tris, hits, quv):
    """the `reserved` word of every record: closest_reference.side_words at the query's point of the pair"""
    return cr.side_words(scene, query_points(tris, quv), hits)


# ---- binary64 -------------------------------------------------------------------------------------------------------------------

def vertices64(tris):
    t = np.asarray(tris, F).reshape(-1, 12).astype(np.float64)
    return t[:, 0:3], t[:, 4:7], t[:, 8:11]


def _normal(A, B, C):
    N = np.cross(B - A, C - A)
    return N, (N * N).sum(-1)


def point_triangle64(p, A, B, C):
    """binary64 (squared distance, nearest point) of points to triangles as convex sets"""
    N, nn = _normal(A, B, C)
    with np.errstate(all="ignore"):
        d2, q, _ = cr._tri_d2_64(p, A, B, C, N, nn)
    return d2, q


def segment_triangle64(E0, E1, A, B, C, iters=64):
    """(d, s, q): the binary64 distance of segments E0..E1 to triangles (A, B, C), a parameter where it is attained and the triangle's
    point there: segment_reference.pair_distance64's ternary search (the distance to a convex set is convex along a line), then the
    better of the search's end and the two endpoints"""
    N, nn = _normal(A, B, C)

    def f(s):
        with np.errstate(all="ignore"):
            d2, q, _ = cr._tri_d2_64(E0 + s[:, None] * (E1 - E0), A, B, C, N, nn)
        return d2, q
    lo, hi = np.zeros(len(E0)), np.ones(len(E0))
    for _ in range(iters):
        m1, m2 = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        left = f(m1)[0] <= f(m2)[0]
        hi = np.where(left, m2, hi); lo = np.where(left, lo, m1)
    s = (lo + hi) / 2
    d2, q = f(s)
    for end in (np.zeros(len(E0)), np.ones(len(E0))):
        e2, eq = f(end)
        take = e2 < d2
        d2 = np.where(take, e2, d2); s = np.where(take, end, s); q = np.where(take[:, None], eq, q)
    return np.sqrt(d2), s, q


def pair_distance64(scene, tris, qi, ti, iters=64, chunk=1 << 17):
    """(d, q) of every pair: the binary64 distance of query triangle qi[k] to scene triangle ti[k] as the minimum over the six
    edge-against-triangle pairs, and the scene triangle's point of that pair"""
    P = vertices64(tris)
    d_out, q_out = np.full(len(qi), np.inf), np.zeros((len(qi), 3))
    for k0 in range(0, len(qi), chunk):
        a, b = qi[k0:k0 + chunk], ti[k0:k0 + chunk]
        Q = tuple(p[a] for p in P)
        S = (scene.A[b], scene.B[b], scene.C[b])
        d, q = np.full(len(a), np.inf), np.zeros((len(a), 3))
        for i, j in Q_EDGES:     # the query's edge against the scene triangle: the scene's point is the triangle's
            dd, _, qq = segment_triangle64(Q[i], Q[j], S[0], S[1], S[2], iters)
            take = dd < d
            d = np.where(take, dd, d); q = np.where(take[:, None], qq, q)
        for i, j in S_EDGES:     # the scene triangle's edge against the query: the scene's point is the edge's
            dd, s, _ = segment_triangle64(S[i], S[j], Q[0], Q[1], Q[2], iters)
            take = dd < d
            d = np.where(take, dd, d); q = np.where(take[:, None], S[i] + s[:, None] * (S[j] - S[i]), q)
        d_out[k0:k0 + chunk] = d; q_out[k0:k0 + chunk] = q
    return d_out, q_out


def candidate_pairs(scene, tris, cull_mask=0xFF, reach=1e-3, chunk=1 << 21):
    """(query index, triangle index) arrays, sorted by query: the valid records against the admitted triangles that can be the nearest
    or a runner-up.  Upper bound per record: the smallest distance of a real pair (the query's vertices to a triangle, a triangle's
    vertices to the query) and, in a second round, of a 12-step ternary search over the survivors.  Lower bound per pair: the distance of
    the scene triangle's centroid to the query triangle minus the scene triangle's radius."""
    P0, P1, P2 = vertices64(tris)
    ok = valid_triangles(tris)
    tri = np.nonzero(scene.admitted(cull_mask))[0]
    if len(tri) == 0 or not ok.any():
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    A, B, C = scene.A[tri], scene.B[tri], scene.C[tri]
    cen = (A + B + C) / 3
    rad = np.sqrt(np.maximum(np.maximum(((A - cen) ** 2).sum(-1), ((B - cen) ** 2).sum(-1)), ((C - cen) ** 2).sum(-1)))
    fin = np.isfinite(cen).all(axis=1) & np.isfinite(rad)
    tri, cen, rad, A, B, C = tri[fin], cen[fin], rad[fin], A[fin], B[fin], C[fin]
    mag_t = float(np.abs(cen).max() + rad.max()) if len(tri) else 0.0
    qi, ti = [], []
    idx = np.nonzero(ok)[0]
    per = max(1, chunk // max(1, len(tri)))
    for k0 in range(0, len(idx), per):
        i = idx[k0:k0 + per]
        Q = (P0[i, None], P1[i, None], P2[i, None])
        lb = np.sqrt(point_triangle64(cen[None], *Q)[0]) - rad[None]
        ub = np.full(lb.shape, np.inf)
        for p in Q:
            ub = np.minimum(ub, point_triangle64(p, A[None], B[None], C[None])[0])
        for p in (A, B, C):
            ub = np.minimum(ub, point_triangle64(p[None], *Q)[0])
        mag = np.maximum(np.abs(np.concatenate([P0[i], P1[i], P2[i]], axis=1)).max(axis=1), mag_t)
        margin = 1e-5 * mag
        first = lb <= (np.sqrt(ub.min(axis=1)) * (1 + reach) + margin)[:, None]
        r, c = np.nonzero(first)
        d, _ = pair_distance64(scene, np.asarray(tris, F).reshape(-1, 12), i[r], tri[c], iters=12)
        best = np.full(len(i), np.inf)
        np.minimum.at(best, r, d)
        keep = lb[r, c] <= best[r] * (1 + reach) + margin[r]
        qi.append(i[r[keep]]); ti.append(tri[c[keep]])
    return np.concatenate(qi), np.concatenate(ti)


def brute64(scene, tris, cull_mask=0xFF, picked=None, pairs=None):
    """binary64 over the candidate pairs; the dict of segment_reference.brute64 with the query triangle in the segment's place: t, inst,
    prim, tri (nearest; -1 without any triangle), q (the scene's point of a nearest pair), runner (the distance of the nearest triangle
    that does NOT touch q; inf without one), touching (how many triangles touch q), picked_touches and picked_t (with picked = (inst,
    prim) arrays: that triangle touches q; its own binary64 distance to the query, inf when it is no candidate), level and runner_level
    (how many triangles are as near as the nearest within 8 x 2^-24 of the magnitude, and the distance of the nearest one that is not),
    mag (largest coordinate magnitude of the query and the nearest triangle).  r_max is not applied."""
    P0, P1, P2 = vertices64(tris)
    n = len(P0)
    res = dict(t=np.full(n, np.inf), inst=np.full(n, -1, np.int64), prim=np.full(n, -1, np.int64), q=np.zeros((n, 3)),
               runner=np.full(n, np.inf), touching=np.zeros(n, np.int64), picked_touches=np.zeros(n, bool), picked_t=np.full(n, np.inf),
               mag=np.zeros(n), tri=np.full(n, -1, np.int64), level=np.zeros(n, np.int64), runner_level=np.full(n, np.inf))
    qi, ti = candidate_pairs(scene, tris, cull_mask) if pairs is None else pairs
    if len(qi) == 0:
        return res
    d, q = pair_distance64(scene, tris, qi, ti)
    order = np.lexsort((ti, d, qi))
    q_sorted = qi[order]
    head = np.concatenate([[True], q_sorted[1:] != q_sorted[:-1]])
    rows, pos = q_sorted[head], order[head]
    res["t"][rows] = d[pos]; res["q"][rows] = q[pos]; res["tri"][rows] = ti[pos]
    res["inst"][rows] = scene.inst[ti[pos]]; res["prim"][rows] = scene.prim[ti[pos]]
    k = ti[pos]
    tri_mag = np.maximum(np.maximum(np.abs(scene.A[k]).max(-1), np.abs(scene.B[k]).max(-1)), np.abs(scene.C[k]).max(-1))
    res["mag"][rows] = np.maximum(np.abs(np.concatenate([P0[rows], P1[rows], P2[rows]], axis=1)).max(axis=1), tri_mag)
    dq, _ = point_triangle64(res["q"][qi], scene.A[ti], scene.B[ti], scene.C[ti])
    touch = np.sqrt(dq) <= 8 * 2.0 ** -24 * res["mag"][qi]
    res["touching"] = np.bincount(qi[touch], minlength=n)
    np.minimum.at(res["runner"], qi, np.where(touch, np.inf, d))
    level = d <= res["t"][qi] + 8 * 2.0 ** -24 * res["mag"][qi]
    res["level"] = np.bincount(qi[level], minlength=n)
    np.minimum.at(res["runner_level"], qi, np.where(level, np.inf, d))
    if picked is not None:
        first = np.concatenate([[0], np.cumsum(np.bincount(scene.inst, minlength=len(scene.mask)))])
        pi, pp = np.asarray(picked[0], np.int64), np.asarray(picked[1], np.int64)
        g = np.where(pi >= 0, first[np.clip(pi, 0, None)] + pp, -1)
        mine = ti == g[qi]
        res["picked_touches"][qi[mine]] = touch[mine]
        res["picked_t"][qi[mine]] = d[mine]
    return res


def altproj64(scene, tris, qi, ti, rounds=200):
    """the distance of the point pair that `rounds` rounds of alternating binary64 projections reach from the query's centroid: onto
    the scene triangle, back onto the query, and so on.  A real pair: an upper bound on the distance of the two triangles."""
    P0, P1, P2 = (p[qi] for p in vertices64(tris))
    A, B, C = scene.A[ti], scene.B[ti], scene.C[ti]
    x = (P0 + P1 + P2) / 3
    y = x
    for _ in range(rounds):
        _, y = point_triangle64(x, A, B, C)
        _, x = point_triangle64(y, P0, P1, P2)
    return np.sqrt(((x - y) ** 2).sum(-1))
