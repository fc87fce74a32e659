"""Two references for rt_closest_segment_device (include/rt_api.h; DESIGN.md §5 "Closest points of segments"), neither with a tree:

 * brute32: the canonical binary32 feature sequence and the key (d2, inst, prim) restated in numpy from the header and DESIGN text, over
   every triangle of every admitted instance, with the exactly rounded binary32 fma, the Scene class, the closest-point sequence and the
   side words of tests/closest_reference.py.  The GPU is held to it byte for byte.
 * brute64: an independent binary64 distance on the same binary32 inputs: the binary64 point-to-triangle distance of
   closest_reference (the triangle as a convex set) minimised over the segment's parameter s.  That distance is convex in s, so a
   ternary search plus both endpoints finds it; the feature list of brute32 is NOT restated.

candidate_pairs() is a conservative pre-filter for brute64 (bounding spheres in binary64 with margins): it only drops pairs that can be
neither the nearest nor a runner-up within the identity rule's reach."""
import numpy as np

from tests import closest_reference as cr
from tests.closest_reference import F, cross3, dot3
from vulkan_raytracing_amd.api import HIT_DTYPE


def valid_segments(segs):
    """(n,) bool: finite endpoints and r_max >= 0 (a NaN r_max fails)"""
    s = np.asarray(segs, F).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        return np.isfinite(s[:, 0:3]).all(axis=1) & np.isfinite(s[:, 4:7]).all(axis=1) & (s[:, 3] >= 0)


# ---- binary32: the canonical sequence -------------------------------------------------------------------------------------------

def clamp(x):
    """the canonical clamp to [0, 1]: NaN and -0 give +0"""
    with np.errstate(invalid="ignore"):
        return np.where(x > 0, np.where(x < 1, x, F(1)), F(0)).astype(F)


def _take(state, d2, uu, vv, ss, allow):
    """a later feature replaces an earlier one only when its d2 is strictly smaller; a NaN d2 is skipped"""
    best, u, v, s = state
    with np.errstate(invalid="ignore"):
        m = allow & ~np.isnan(d2) & ~(d2 >= best)
    return np.where(m, d2, best), np.where(m, uu, u), np.where(m, vv, v), np.where(m, ss, s)


def seg_tri32(P0, P1, a, ab, ac):
    """the canonical (d2, u, v, s) of segments P0..P1 against triangles (a, ab, ac): tuples of three broadcastable float32 arrays.
    d2 is NaN where no feature has a value."""
    with np.errstate(all="ignore"):
        d = tuple(P1[k] - P0[k] for k in range(3))
        shape = np.broadcast(P0[0], a[0]).shape
        point = np.broadcast_to((P0[0] == P1[0]) & (P0[1] == P1[1]) & (P0[2] == P1[2]), shape)
        zero, one = np.zeros(shape, F), np.ones(shape, F)
        state = (np.full(shape, np.nan, F), zero, zero, zero)
        # 1, 2: the endpoints
        d2, u, v = cr.tri_d2(P0, a, ab, ac)
        state = _take(state, d2, u, v, zero, np.ones(shape, bool))
        d2, u, v = cr.tri_d2(P1, a, ab, ac)
        state = _take(state, d2, u, v, one, ~point)
        # 3: the plane crossing
        n = cross3(ab, ac)
        h0 = dot3(n, tuple(P0[k] - a[k] for k in range(3)))
        h1 = dot3(n, tuple(P1[k] - a[k] for k in range(3)))
        exists = ((h0 < 0) & (h1 > 0)) | ((h0 > 0) & (h1 < 0))
        s = clamp(h0 / (h0 - h1))
        X = tuple(P0[k] + s * d[k] for k in range(3))
        d2, u, v = cr.tri_d2(X, a, ab, ac)
        state = _take(state, d2, u, v, s, exists & ~point)
        # 4: the edges AB, AC, BC
        A = dot3(d, d)
        b = tuple(a[k] + ab[k] for k in range(3))
        bc = tuple(ac[k] - ab[k] for k in range(3))
        for q, e, which in ((a, ab, 0), (a, ac, 1), (b, bc, 2)):
            r = tuple(P0[k] - q[k] for k in range(3))
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
            w = tuple((P0[k] + ss * d[k]) - (q[k] + tt * e[k]) for k in range(3))
            d2 = dot3(w, w)
            uu = tt if which == 0 else (zero if which == 1 else F(1) - tt)
            vv = zero if which == 0 else tt
            state = _take(state, d2, uu, vv, ss, ~point)
        return tuple(np.asarray(x, F) for x in state)


def brute32(scene, segs, cull_mask=0xFF, chunk=1 << 19):
    """(HIT_DTYPE records, s float32): the smallest key (d2, inst, prim) over the admitted triangles whose d2 is not NaN and is
    <= r_max * r_max, t = sqrt(d2); the miss record (t = r_max as given, s = 0) otherwise and for invalid records"""
    sg = np.ascontiguousarray(segs, F).reshape(-1, 8)
    n = len(sg)
    out = np.zeros(n, HIT_DTYPE)
    out["t"] = sg[:, 3]; out["prim"] = -1; out["inst"] = -1
    s_out = np.zeros(n, F)
    with np.errstate(all="ignore"):
        r2 = sg[:, 3] * sg[:, 3]
    tri = np.nonzero(scene.admitted(cull_mask))[0]
    idx = np.nonzero(valid_segments(sg))[0]
    if len(tri) == 0:
        return out, s_out
    per = max(1, chunk // len(tri))
    ta, tab, tac = (tuple(getattr(scene, name)[tri, k][None, :] for k in range(3)) for name in ("a", "ab", "ac"))
    for k0 in range(0, len(idx), per):
        i = idx[k0:k0 + per]
        d2, u, v, s = seg_tri32(tuple(sg[i, k][:, None] for k in range(3)), tuple(sg[i, 4 + k][:, None] for k in range(3)), ta, tab, tac)
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
        s_out[ii] = s[rr, jj]
    return out, s_out


def segment_points(segs, s):
    """(n, 4) float32 point records P0 + s d, d = P1 - P0 (per component one product and one sum), with the records' r_max"""
    sg = np.asarray(segs, F).reshape(-1, 8)
    with np.errstate(all="ignore"):
        p = sg[:, 0:3] + np.asarray(s, F)[:, None] * (sg[:, 4:7] - sg[:, 0:3])
    return np.concatenate([p, sg[:, 3:4]], axis=1).astype(F)


def side_words(scene, segs, hits, s):
    """the `reserved` word of every record: closest_reference.side_words at p = P0 + s d"""
    return cr.side_words(scene, segment_points(segs, s), hits)


# ---- binary64: the minimum over s of the point-to-triangle distance ---------------------------------------------------------------

def _seg_point_d(p, a, b):
    """binary64 distances from points p to segments a..b (last axis: x, y, z)"""
    d2, _ = cr._segment_d2(p, a, b)
    return np.sqrt(d2)


def candidate_pairs(scene, segs, cull_mask=0xFF, reach=1e-3, chunk=1 << 22):
    """(segment index, triangle index) arrays, sorted by segment: the valid segments against the admitted triangles whose bounding sphere
    is no farther from the segment than (1 + reach) times the smallest centroid distance of any triangle, plus 1e-5 of the magnitudes"""
    sg = np.asarray(segs, F).reshape(-1, 8).astype(np.float64)
    ok = valid_segments(segs)
    tri = np.nonzero(scene.admitted(cull_mask))[0]
    if len(tri) == 0 or not ok.any():
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    A, B, C = scene.A[tri], scene.B[tri], scene.C[tri]
    cen = (A + B + C) / 3
    rad = np.sqrt(np.maximum(np.maximum(((A - cen) ** 2).sum(-1), ((B - cen) ** 2).sum(-1)), ((C - cen) ** 2).sum(-1)))
    fin = np.isfinite(cen).all(axis=1) & np.isfinite(rad)
    tri, cen, rad = tri[fin], cen[fin], rad[fin]
    mag_t = float(np.abs(cen).max() + rad.max()) if len(tri) else 0.0
    si, ti = [], []
    idx = np.nonzero(ok)[0]
    per = max(1, chunk // max(1, len(tri)))
    for k0 in range(0, len(idx), per):
        i = idx[k0:k0 + per]
        dc = _seg_point_d(cen[None], sg[i, None, 0:3], sg[i, None, 4:7])
        mag = np.maximum(np.abs(sg[i][:, [0, 1, 2, 4, 5, 6]]).max(axis=1), mag_t)
        ub = dc.min(axis=1) * (1 + reach) + 1e-5 * mag
        a, b = np.nonzero(dc - rad[None] <= ub[:, None])
        si.append(i[a]); ti.append(tri[b])
    return np.concatenate(si), np.concatenate(ti)


def pair_distance64(scene, segs, si, ti, iters=64, chunk=1 << 18):
    """(d, s, q) of every pair: the binary64 distance of segment si[k] to triangle ti[k], a parameter s where it is attained and the
    triangle's point q there.  Ternary search over s in [0, 1] (the distance to a convex set is convex along a line), then the better
    of the search's end and the two endpoints."""
    sg = np.asarray(segs, F).reshape(-1, 8).astype(np.float64)
    d_out, s_out, q_out = np.zeros(len(si)), np.zeros(len(si)), np.zeros((len(si), 3))
    for k0 in range(0, len(si), chunk):
        a, b = si[k0:k0 + chunk], ti[k0:k0 + chunk]
        P0, P1 = sg[a, 0:3], sg[a, 4:7]
        A, B, C = scene.A[b], scene.B[b], scene.C[b]
        N = np.cross(B - A, C - A)
        nn = (N * N).sum(-1)

        def f(s):
            with np.errstate(all="ignore"):
                d2, q, _ = cr._tri_d2_64(P0 + s[:, None] * (P1 - P0), A, B, C, N, nn)
            return d2, q
        lo, hi = np.zeros(len(a)), np.ones(len(a))
        for _ in range(iters):
            m1, m2 = lo + (hi - lo) / 3, hi - (hi - lo) / 3
            left = f(m1)[0] <= f(m2)[0]
            hi = np.where(left, m2, hi); lo = np.where(left, lo, m1)
        s = (lo + hi) / 2
        d2, q = f(s)
        for end in (np.zeros(len(a)), np.ones(len(a))):
            e2, eq = f(end)
            take = e2 < d2
            d2 = np.where(take, e2, d2); s = np.where(take, end, s); q = np.where(take[:, None], eq, q)
        d_out[k0:k0 + chunk] = np.sqrt(d2); s_out[k0:k0 + chunk] = s; q_out[k0:k0 + chunk] = q
    return d_out, s_out, q_out


def brute64(scene, segs, cull_mask=0xFF, picked=None, pairs=None):
    """binary64 over the candidate pairs.  dict: t, inst, prim (nearest; -1 without any triangle), s and q (a nearest pair's parameter and
    surface point), runner (the distance of the nearest triangle that does NOT touch q: triangles that share the vertex or edge q lies
    on are at the same distance by construction; inf without one), touching (how many triangles touch q), picked_touches and picked_t
    (with picked = (inst, prim) arrays: that triangle touches q; its own binary64 distance to the segment, inf when it is no candidate),
    level and runner_level (how many triangles are as near as the nearest within 8 x 2^-24 of the magnitude, and the distance of the
    nearest one that is not: `touching` and `runner` by distance alone, for segments whose nearest pair is not unique), mag (largest coordinate magnitude of the segment and the nearest triangle).  r_max is not applied."""
    sg = np.asarray(segs, F).reshape(-1, 8).astype(np.float64)
    n = len(sg)
    res = dict(t=np.full(n, np.inf), inst=np.full(n, -1, np.int64), prim=np.full(n, -1, np.int64), s=np.zeros(n), q=np.zeros((n, 3)),
               runner=np.full(n, np.inf), touching=np.zeros(n, np.int64), picked_touches=np.zeros(n, bool), picked_t=np.full(n, np.inf),
               mag=np.zeros(n), tri=np.full(n, -1, np.int64), level=np.zeros(n, np.int64), runner_level=np.full(n, np.inf))
    si, ti = candidate_pairs(scene, segs, cull_mask) if pairs is None else pairs
    if len(si) == 0:
        return res
    d, s, q = pair_distance64(scene, segs, si, ti)
    order = np.lexsort((ti, d, si))
    s_sorted = si[order]
    head = np.concatenate([[True], s_sorted[1:] != s_sorted[:-1]])
    rows, pos = s_sorted[head], order[head]
    res["t"][rows] = d[pos]; res["s"][rows] = s[pos]; res["q"][rows] = q[pos]; res["tri"][rows] = ti[pos]
    res["inst"][rows] = scene.inst[ti[pos]]; res["prim"][rows] = scene.prim[ti[pos]]
    k = ti[pos]
    tri_mag = np.maximum(np.maximum(np.abs(scene.A[k]).max(-1), np.abs(scene.B[k]).max(-1)), np.abs(scene.C[k]).max(-1))
    res["mag"][rows] = np.maximum(np.abs(sg[rows][:, [0, 1, 2, 4, 5, 6]]).max(axis=1), tri_mag)
    # which candidates touch the nearest point (a few binary32 ulps of the magnitude, as closest_reference.brute64 has it)
    A, B, C = scene.A[ti], scene.B[ti], scene.C[ti]
    N = np.cross(B - A, C - A)
    with np.errstate(all="ignore"):
        dq, _, _ = cr._tri_d2_64(res["q"][si], A, B, C, N, (N * N).sum(-1))
    touch = np.sqrt(dq) <= 8 * 2.0 ** -24 * res["mag"][si]
    res["touching"] = np.bincount(si[touch], minlength=n)
    far = np.where(touch, np.inf, d)
    np.minimum.at(res["runner"], si, far)
    # the same by distance alone, for segments whose nearest pair is a continuum (parallel to an edge, in a triangle's plane): the
    # candidates as near as the nearest one within that threshold, and the nearest one beyond it
    level = d <= res["t"][si] + 8 * 2.0 ** -24 * res["mag"][si]
    res["level"] = np.bincount(si[level], minlength=n)
    np.minimum.at(res["runner_level"], si, np.where(level, np.inf, d))
    if picked is not None:
        first = np.concatenate([[0], np.cumsum(np.bincount(scene.inst, minlength=len(scene.mask)))])
        pi, pp = np.asarray(picked[0], np.int64), np.asarray(picked[1], np.int64)
        g = np.where(pi >= 0, first[np.clip(pi, 0, None)] + pp, -1)
        mine = ti == g[si]
        res["picked_touches"][si[mine]] = touch[mine]
        res["picked_t"][si[mine]] = d[mine]
    return res
