"""Two references for rt_sweep_spheres_device (include/rt_api.h; DESIGN.md §5 "Sphere sweeps"), neither with a tree:

 * brute32: the canonical binary32 contact time and the key (t, inst, prim) restated in numpy from the header and DESIGN text, with the
   exactly rounded binary32 fma of tests/closest_reference.py for the library's fused operations.  The GPU is held to it byte for byte.
 * brute64: the exact first-contact time in binary64 on the same binary32 inputs: the minimum over the face, the three edge cylinders
   and the three vertex spheres, each solved about its own closest approach; 0 when the distance at o is <= r, +inf without a contact.

Both run over (sweep, triangle) pairs.  candidate_pairs() is a conservative pre-filter (binary64 slab tests of the centre's path
against the triangles' bounding boxes, inflated by the radius and a margin far above anything binary32 can add); it only drops pairs
that cannot touch, and either reference over the survivors equals the same reference over every pair."""
import numpy as np

from tests import closest_reference as cr
from tests.closest_reference import F, cross3, dot3
from vulkan_raytracing_amd.api import HIT_DTYPE

INF32 = F(np.inf)
SW_FACE = F(2.0 ** -20)   # the face contact's residual bound, squared: (2^-10 of the longer edge)^2


def valid_sweeps(sweeps):
    """(n,) bool: finite o, r and d, r >= 0, d != 0, tmax >= 0 (a NaN tmax fails)"""
    s = np.asarray(sweeps, F).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        return np.isfinite(s[:, 0:7]).all(axis=1) & (s[:, 3] >= 0) & (s[:, 4:7] != 0).any(axis=1) & (s[:, 7] >= 0)


def _slab(o, d, tmax, lo, hi):
    """binary64: the path o + t d, t in [0, tmax], meets the box [lo, hi] (last axis: x, y, z)"""
    with np.errstate(all="ignore"):
        inv = 1.0 / d
        t1, t2 = (lo - o) * inv, (hi - o) * inv
        par = d == 0
        inside = (o >= lo) & (o <= hi)
        tn = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2))
        tf = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2))
        return np.maximum(tn.max(-1), 0.0) <= np.minimum(tf.min(-1), tmax)


def candidate_pairs(scene, sweeps, cull_mask=0xFF, extra=0.0, chunk=1 << 22):
    """(sweep index, triangle index) arrays, sorted by sweep: the valid sweeps against the admitted triangles whose bounding box, inflated
    by 1.01 r + extra + 2 % of the scene's extent + 1e-4 of the largest magnitude, the centre's path meets"""
    s = np.asarray(sweeps, F).reshape(-1, 8).astype(np.float64)
    ok = valid_sweeps(sweeps)
    n = len(s)
    if scene.n_tris == 0 or not ok.any():
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    lo_t = np.minimum(np.minimum(scene.A, scene.B), scene.C)
    hi_t = np.maximum(np.maximum(scene.A, scene.B), scene.C)
    fin = np.isfinite(lo_t).all(axis=1) & np.isfinite(hi_t).all(axis=1)
    lo, hi = lo_t[fin].min(axis=0), hi_t[fin].max(axis=0)
    o, d, tmax = s[:, 0:3], s[:, 4:7], s[:, 7]
    with np.errstate(invalid="ignore"):
        mag = np.maximum(np.abs(np.where(ok[:, None], o, 0.0)).max(axis=1), max(np.abs(lo).max(), np.abs(hi).max()))
        R = np.where(ok, 1.01 * s[:, 3] + extra + 0.02 * (hi - lo).max() + 1e-4 * mag, 0.0)
    first = np.concatenate([[0], np.cumsum(np.bincount(scene.inst, minlength=len(scene.mask)))])
    si, ti = [], []
    for ii in range(len(scene.mask)):
        f, c = first[ii], first[ii + 1] - first[ii]
        if c == 0 or (scene.mask[ii] & cull_mask) == 0:
            continue
        tl, th = lo_t[f:f + c], hi_t[f:f + c]
        keep = np.nonzero(fin[f:f + c])[0]
        if len(keep) == 0:
            continue
        tl, th = tl[keep], th[keep]
        idx = np.nonzero(ok & _slab(o, d, tmax, tl.min(axis=0)[None] - R[:, None], th.max(axis=0)[None] + R[:, None]))[0]
        per = max(1, chunk // len(keep))
        for k0 in range(0, len(idx), per):
            j = idx[k0:k0 + per]
            hit = _slab(o[j, None, :], d[j, None, :], tmax[j, None], tl[None] - R[j, None, None], th[None] + R[j, None, None])
            a, b = np.nonzero(hit)
            si.append(j[a]); ti.append(f + keep[b])
    if not si:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    si, ti = np.concatenate(si), np.concatenate(ti)
    order = np.lexsort((ti, si))
    return si[order], ti[order]


# ---- binary32: the canonical sequence -------------------------------------------------------------------------------------------

def _take(tc, tp, tmax, uu, vv, ok, t, u, v):
    """sweep_take: the root tc + tp replaces (t, u, v) when the feature accepted it, it lies in [0, tmax] and it precedes t"""
    tt = tc + tp
    m = ok & (tt >= 0) & (tt <= tmax) & (tt < t)
    return np.where(m, tt, t), np.where(m, uu, u), np.where(m, vv, v)


def _edge(m, e, d, dd, rr):
    ee, me, de, md, mm = dot3(e, e), dot3(m, e), dot3(d, e), dot3(m, d), dot3(m, m)
    a = ee * dd - de * de
    b = ee * md - de * me
    c = ee * (mm - rr) - me * me
    disc = b * b - a * c
    tp = (-b - np.sqrt(disc)) / a
    s = (me + tp * de) / ee
    return tp, s, (a > 0) & (disc >= 0) & (s >= 0) & (s <= 1)


def _vertex(m, d, dd, rr):
    b, c = dot3(m, d), dot3(m, m) - rr
    disc = b * b - dd * c
    tp = (-b - np.sqrt(disc)) / dd
    return tp, (dd > 0) & (disc >= 0)


def sweep_tri32(o, r, d, tmax, A, ab, ac):
    """the canonical contact of sweeps (o, r, d, tmax) with triangles (A, ab, ac): tuples of three float32 arrays (vectors) and float32
    arrays of one shape.  Returns (found, t, u, v)."""
    with np.errstate(all="ignore"):
        finite = np.ones(np.shape(r), bool)
        for vec in (A, ab, ac):
            for k in range(3):
                finite = finite & np.isfinite(vec[k])
        rr, dd = r * r, dot3(d, d)
        d2, u0, v0 = cr.tri_d2(o, A, ab, ac)
        overlap = d2 <= rr
        tc = dot3(tuple(A[k] - o[k] for k in range(3)), d) / dd
        tc = np.where(tc >= 0, tc, F(0))
        tc = np.where(tc > tmax, tmax, tc)
        oc = tuple(o[k] + tc * d[k] for k in range(3))
        mp = tuple(oc[k] - A[k] for k in range(3))
        # face
        n = cross3(ab, ac)
        nn, nd = dot3(n, n), dot3(n, d)
        flip = nd > 0
        n = tuple(np.where(flip, -n[k], n[k]) for k in range(3))
        nd = np.where(flip, -nd, nd)
        sn = np.sqrt(nn)
        tpf = (r * sn - dot3(n, mp)) / nd
        kk = r / sn
        q = tuple((mp[k] + tpf * d[k]) - kk * n[k] for k in range(3))
        d00, d01, d11, d20, d21 = dot3(ab, ab), dot3(ab, ac), dot3(ac, ac), dot3(q, ab), dot3(q, ac)
        den = d00 * d11 - d01 * d01
        bv = (d11 * d20 - d01 * d21) / den
        bw = (d00 * d21 - d01 * d20) / den
        cq = tuple(q[k] - (bv * ab[k] + bw * ac[k]) for k in range(3))
        tf = tc + tpf
        face = (nn > 0) & (nd < 0) & (bv >= 0) & (bw >= 0) & (bv + bw <= 1) & (dot3(cq, cq) <= SW_FACE * np.maximum(d00, d11)) & (tf >= 0) & (tf <= tmax)
        # edges AB, AC, BC, vertices A, B, C
        zero, one = np.zeros_like(tc), np.ones_like(tc)
        t = np.full(np.shape(tc), INF32)
        u, v = zero, zero
        tp, s, ok = _edge(mp, ab, d, dd, rr)
        t, u, v = _take(tc, tp, tmax, s, zero, ok, t, u, v)
        tp, s, ok = _edge(mp, ac, d, dd, rr)
        t, u, v = _take(tc, tp, tmax, zero, s, ok, t, u, v)
        mb = tuple(mp[k] - ab[k] for k in range(3))
        mc = tuple(mp[k] - ac[k] for k in range(3))
        tp, s, ok = _edge(mb, tuple(ac[k] - ab[k] for k in range(3)), d, dd, rr)
        t, u, v = _take(tc, tp, tmax, F(1) - s, s, ok, t, u, v)
        tp, ok = _vertex(mp, d, dd, rr)
        t, u, v = _take(tc, tp, tmax, zero, zero, ok, t, u, v)
        tp, ok = _vertex(mb, d, dd, rr)
        t, u, v = _take(tc, tp, tmax, one, zero, ok, t, u, v)
        tp, ok = _vertex(mc, d, dd, rr)
        t, u, v = _take(tc, tp, tmax, zero, one, ok, t, u, v)
        found = finite & (overlap | face | (t < INF32))
        t = np.where(overlap, F(0), np.where(face, tf, t))
        u = np.where(overlap, u0, np.where(face, bv, u))
        v = np.where(overlap, v0, np.where(face, bw, v))
        return found, t.astype(F), u.astype(F), v.astype(F)


def _first_per_sweep(si, keys):
    """the position of the smallest key tuple (major key first) of every sweep that has one: (sweeps, positions)"""
    order = np.lexsort(tuple(reversed(keys)) + (si,))
    s_sorted = si[order]
    head = np.concatenate([[True], s_sorted[1:] != s_sorted[:-1]]) if len(order) else np.zeros(0, bool)
    return s_sorted[head], order[head]


def pair_contacts32(scene, sweeps, si, ti, chunk=1 << 18):
    """(found, t, u, v) of every pair"""
    s = np.ascontiguousarray(sweeps, F).reshape(-1, 8)
    out = [np.zeros(len(si), bool)] + [np.zeros(len(si), F) for _ in range(3)]
    for k0 in range(0, len(si), chunk):
        a, b = si[k0:k0 + chunk], ti[k0:k0 + chunk]
        res = sweep_tri32(tuple(s[a, k] for k in range(3)), s[a, 3], tuple(s[a, 4 + k] for k in range(3)), s[a, 7],
                          tuple(scene.a[b, k] for k in range(3)), tuple(scene.ab[b, k] for k in range(3)), tuple(scene.ac[b, k] for k in range(3)))
        for o_, r_ in zip(out, res):
            o_[k0:k0 + chunk] = r_
    return out


def brute32(scene, sweeps, cull_mask=0xFF, pairs=None):
    """HIT_DTYPE records: the smallest key (t, inst, prim) over the admitted triangles with a canonical contact; the miss record (t = tmax
    as given) otherwise and for invalid records"""
    s = np.ascontiguousarray(sweeps, F).reshape(-1, 8)
    out = np.zeros(len(s), HIT_DTYPE)
    out["t"] = s[:, 7]; out["prim"] = -1; out["inst"] = -1
    si, ti = candidate_pairs(scene, s, cull_mask) if pairs is None else pairs
    if len(si) == 0:
        return out
    found, t, u, v = pair_contacts32(scene, s, si, ti)
    si, ti, t, u, v = si[found], ti[found], t[found], u[found], v[found]
    rows, pos = _first_per_sweep(si, (t, scene.inst[ti], scene.prim[ti]))
    out["t"][rows] = t[pos]; out["u"][rows] = u[pos]; out["v"][rows] = v[pos]
    out["prim"][rows] = scene.prim[ti[pos]]; out["inst"][rows] = scene.inst[ti[pos]]
    return out


def side_words(scene, sweeps, hits):
    """the `reserved` word of every record: closest_reference.side_words at p = o + t d (per component one product and one sum)"""
    s = np.asarray(sweeps, F).reshape(-1, 8)
    with np.errstate(all="ignore"):
        p = s[:, 0:3] + hits["t"][:, None] * s[:, 4:7]
    return cr.side_words(scene, np.concatenate([p, np.zeros((len(s), 1), F)], axis=1), hits)


# ---- binary64: the exact first contact ------------------------------------------------------------------------------------------

def _dots(a, b):
    return (a * b).sum(-1)


def contact64(o, r, d, A, B, C):
    """(pairs,) the first t >= 0 at which the sphere (o + t d, r) touches triangle ABC; 0 when it does at t = 0; +inf for none.  Every
    feature is solved about its own closest approach, so nothing cancels beyond binary64's own rounding."""
    with np.errstate(all="ignore"):
        ab, ac = B - A, C - A
        N = np.cross(ab, ac)
        nn = _dots(N, N)
        d2, _, _ = cr._tri_d2_64(o, A, B, C, N, nn)
        dd = _dots(d, d)
        t = np.full(len(o), np.inf)
        # face
        nd = _dots(N, d)
        sgn = np.where(nd > 0, -1.0, 1.0)
        n, nd = N * sgn[:, None], nd * sgn
        sn = np.sqrt(nn)
        tf = (r * sn - _dots(n, o - A)) / nd
        q = (o - A) + tf[:, None] * d - (r / sn)[:, None] * n
        u = _dots(np.cross(q, ac), N) / nn
        v = _dots(np.cross(ab, q), N) / nn
        ok = (nn > 0) & (nd < 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (tf >= 0)
        t = np.where(ok, np.minimum(t, tf), t)
        # edges: in the plane perpendicular to the edge, about the closest approach of the two lines
        for P0, e in ((A, ab), (A, ac), (B, ac - ab)):
            ee = _dots(e, e)
            m = o - P0
            mp = m - (_dots(m, e) / ee)[:, None] * e
            dp = d - (_dots(d, e) / ee)[:, None] * e
            a = _dots(dp, dp)
            t0 = -_dots(mp, dp) / a
            c0 = mp + t0[:, None] * dp
            h2 = r * r - _dots(c0, c0)
            te = t0 - np.sqrt(h2 / a)
            s = _dots(m + te[:, None] * d, e) / ee
            ok = (ee > 0) & (a > 0) & (h2 >= 0) & (s >= 0) & (s <= 1) & (te >= 0)
            t = np.where(ok, np.minimum(t, te), t)
        # vertices: about the closest approach to the vertex
        for V in (A, B, C):
            m = o - V
            t0 = -_dots(m, d) / dd
            c0 = m + t0[:, None] * d
            h2 = r * r - _dots(c0, c0)
            tv = t0 - np.sqrt(h2 / dd)
            ok = (dd > 0) & (h2 >= 0) & (tv >= 0)
            t = np.where(ok, np.minimum(t, tv), t)
        return np.where(d2 <= r * r, 0.0, t)


def distance64(scene, p, ti):
    """(records,) the binary64 distance from point p[i] to triangle ti[i]"""
    A, B, C = scene.A[ti], scene.B[ti], scene.C[ti]
    N = np.cross(B - A, C - A)
    with np.errstate(all="ignore"):
        d2, _, _ = cr._tri_d2_64(np.asarray(p, np.float64), A, B, C, N, _dots(N, N))
    return np.sqrt(d2)


def brute64(scene, sweeps, cull_mask=0xFF, radius=None, pairs=None, chunk=1 << 20):
    """(t, tri): the exact first-contact time of every sweep over the admitted triangles (binary64 on the binary32 inputs; +inf without a
    contact and for invalid records; tmax is NOT applied) and the index of that triangle in the scene's arrays (-1 without one).
    radius: (n,) radii in place of the records'."""
    s = np.asarray(sweeps, F).reshape(-1, 8).astype(np.float64)
    r = s[:, 3] if radius is None else np.asarray(radius, np.float64)
    t_out, tri_out = np.full(len(s), np.inf), np.full(len(s), -1, np.int64)
    si, ti = candidate_pairs(scene, sweeps, cull_mask, extra=float(np.max(np.abs(r - s[:, 3]), initial=0.0))) if pairs is None else pairs
    if len(si) == 0:
        return t_out, tri_out
    t = np.zeros(len(si))
    for k0 in range(0, len(si), chunk):
        a, b = si[k0:k0 + chunk], ti[k0:k0 + chunk]
        t[k0:k0 + chunk] = contact64(s[a, 0:3], r[a], s[a, 4:7], scene.A[b], scene.B[b], scene.C[b])
    hit = np.isfinite(t)
    rows, pos = _first_per_sweep(si[hit], (t[hit],))
    t_out[rows] = t[hit][pos]; tri_out[rows] = ti[hit][pos]
    return t_out, tri_out
