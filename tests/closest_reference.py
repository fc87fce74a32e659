"""Two references for rt_closest_point_device (include/rt_api.h; DESIGN.md §5 "Closest points"), neither with a tree:

 * brute32: the canonical binary32 arithmetic and the key (d2, inst, prim) restated in numpy from the header and DESIGN text, over every
   triangle of every admitted instance.  numpy's float32 +, -, *, / and sqrt are IEEE; the library's explicit fused operations (dot3,
   cross3, xform_point, xform_vec) go through fma32, an exactly rounded binary32 fma.  The GPU is held to it byte for byte.
 * brute64: an independent binary64 minimum over the triangle as a convex set (the face if the projection falls inside, else the three
   segments; a zero-area triangle is its segments), with the runner-up distance and the plane side, to which brute32 is held within
   tolerances.

candidates() is a conservative pre-filter for large scenes (box distances in binary64 with margins); it only drops triangles that cannot
be the answer, and brute32 over the survivors equals brute32 over everything."""
import numpy as np

from vulkan_raytracing_amd.api import HIT_DTYPE

F = np.float32
FRONT, BACK = 0xFE, 0xFF
FLIP = 0x2


def fma32(a, b, c):
    """a * b + c rounded once to binary32: the product is exact in binary64, the sum is rounded to odd there (TwoSum), then to binary32"""
    a, b, c = (np.asarray(x, F).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.int64) & 1) != 0
        fix = np.isfinite(s) & (err != 0) & ~odd
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F)


def dot3(a, b):
    """the library's dot3: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))"""
    return fma32(a[2], b[2], fma32(a[1], b[1], a[0] * b[0]))


def cross3(a, b):
    """the library's cross3: (fma(a.y, b.z, -(a.z * b.y)), fma(a.z, b.x, -(a.x * b.z)), fma(a.x, b.y, -(a.y * b.x)))"""
    return (fma32(a[1], b[2], -(a[2] * b[1])), fma32(a[2], b[0], -(a[0] * b[2])), fma32(a[0], b[1], -(a[1] * b[0])))


def xform_vec(m, p):
    """rows r of the 3x4 matrix m: fma(m[r][2], p.z, fma(m[r][1], p.y, m[r][0] * p.x))"""
    return tuple(fma32(m[4 * r + 2], p[2], fma32(m[4 * r + 1], p[1], m[4 * r] * p[0])) for r in range(3))


def xform_point(m, p):
    """xform_vec's row plus m[r][3]"""
    v = xform_vec(m, p)
    return tuple(v[r] + m[4 * r + 3] for r in range(3))


def world_to_object(o2w):
    """gl_WorldToObjectEXT of an instance record: the cofactor inverse in binary64, rounded once"""
    m = np.asarray(o2w, F).astype(np.float64)
    a, b, c, d, e, f, g, h, i = m[0], m[1], m[2], m[4], m[5], m[6], m[8], m[9], m[10]
    tx, ty, tz = m[3], m[7], m[11]
    c00, c01, c02 = e * i - f * h, c * h - b * i, b * f - c * e
    c10, c11, c12 = f * g - d * i, a * i - c * g, c * d - a * f
    c20, c21, c22 = d * h - e * g, b * g - a * h, a * e - b * d
    det = a * c00 + b * c10 + c * c20
    rr = 1.0 / det
    q = [c00 * rr, c01 * rr, c02 * rr, c10 * rr, c11 * rr, c12 * rr, c20 * rr, c21 * rr, c22 * rr]
    w = np.zeros(12, np.float64)
    w[[0, 1, 2, 4, 5, 6, 8, 9, 10]] = q
    w[3] = -(q[0] * tx + q[1] * ty + q[2] * tz)
    w[7] = -(q[3] * tx + q[4] * ty + q[5] * tz)
    w[11] = -(q[6] * tx + q[7] * ty + q[8] * tz)
    return w.astype(F)


class Scene:
    """every triangle of every instance, in (inst, prim) order: the packet (v0, e1 = v1 - v0, e2 = v2 - v0 in binary32), its world form
    (a, ab, ac: the canonical transforms) and, in binary64, its world vertices"""

    def __init__(self, verts6, idx, ranges, instances):
        verts = np.asarray(verts6, F).reshape(-1)
        idx = np.asarray(idx, np.int64)
        meshes = []
        for ff, fi, pc in ranges:
            ix = idx[fi:fi + 3 * pc].reshape(-1, 3)
            p = verts[ff:].reshape(-1, 6)[:, :3]
            v0, v1, v2 = p[ix[:, 0]], p[ix[:, 1]], p[ix[:, 2]]
            meshes.append((v0, v1 - v0, v2 - v0))
        cols = {k: [] for k in ("inst", "prim", "v0", "e1", "e2", "a", "ab", "ac", "A", "B", "C")}
        self.o2w, self.w2o, self.mask, self.flags = [], [], [], []
        for ii, r in enumerate(instances):
            m = np.asarray(r["transform"], F).reshape(12)
            v0, e1, e2 = meshes[int(r["mesh"])]
            self.o2w.append(m); self.w2o.append(world_to_object(m))
            self.mask.append(int(r["custom_index_and_mask"]) >> 24)
            self.flags.append((int(r["sbt_offset_and_flags"]) >> 24) & 0xF)
            n = len(v0)
            cols["inst"].append(np.full(n, ii, np.int32)); cols["prim"].append(np.arange(n, dtype=np.int32))
            cols["v0"].append(v0); cols["e1"].append(e1); cols["e2"].append(e2)
            cols["a"].append(np.stack(xform_point(m, v0.T), axis=1))
            cols["ab"].append(np.stack(xform_vec(m, e1.T), axis=1))
            cols["ac"].append(np.stack(xform_vec(m, e2.T), axis=1))
            M = m.astype(np.float64).reshape(3, 4)
            for name, q in (("A", v0.astype(np.float64)), ("B", v0.astype(np.float64) + e1), ("C", v0.astype(np.float64) + e2)):
                cols[name].append(q @ M[:, :3].T + M[:, 3])
        for k, v in cols.items():
            setattr(self, k, np.concatenate(v) if v else np.zeros((0, 3)))
        self.mask = np.array(self.mask, np.int64); self.flags = np.array(self.flags, np.int64)
        self.o2w = np.array(self.o2w, F).reshape(-1, 12); self.w2o = np.array(self.w2o, F).reshape(-1, 12)
        self.n_tris = len(self.inst)

    def admitted(self, cull_mask):
        """(triangles,) bool: the triangle's instance has (mask & cull_mask) != 0"""
        return (self.mask[self.inst] & cull_mask) != 0 if self.n_tris else np.zeros(0, bool)


def tri_d2(p, a, ab, ac):
    """the canonical d2, u, v of point(s) p against triangle(s) (a, ab, ac): tuples of three broadcastable float32 arrays"""
    with np.errstate(all="ignore"):
        ap = tuple(p[k] - a[k] for k in range(3))
        d1, d2 = dot3(ab, ap), dot3(ac, ap)
        bp = tuple(ap[k] - ab[k] for k in range(3))
        d3, d4 = dot3(ab, bp), dot3(ac, bp)
        cp = tuple(ap[k] - ac[k] for k in range(3))
        d5, d6 = dot3(ab, cp), dot3(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        one, zero = np.ones_like(d1), np.zeros_like(d1)
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = F(1.0) / ((va + vb) + vc)
        u = np.select(conds, [zero, one, d1 / (d1 - d3), zero, zero, F(1.0) - w_bc], vb * denom)
        v = np.select(conds, [zero, zero, zero, one, d2 / (d2 - d6), w_bc], vc * denom)
        c = tuple(ap[k] - (u * ab[k] + v * ac[k]) for k in range(3))
        return dot3(c, c), u, v


def side_words(scene, points, hits):
    """the `reserved` word of every record: FRONT when s = dot(cross(e1, e2), xform_point(w2o, p) - v0) < 0, inverted by FLIP_FACING, 0
    on a miss; also returns s (binary32)"""
    pts = np.asarray(points, F).reshape(-1, 4)
    kinds = np.zeros(len(pts), np.uint32)
    s_out = np.zeros(len(pts), F)
    hit = np.nonzero(hits["inst"] >= 0)[0]
    if len(hit) == 0:
        return kinds, s_out
    first = np.concatenate([[0], np.cumsum(np.bincount(scene.inst, minlength=len(scene.mask)))])
    k = first[hits["inst"][hit]] + hits["prim"][hit]
    w = scene.w2o[hits["inst"][hit]].T
    po = xform_point(w, pts[hit, :3].T)
    v0, e1, e2 = scene.v0[k].T, scene.e1[k].T, scene.e2[k].T
    with np.errstate(all="ignore"):
        s = dot3(cross3(e1, e2), tuple(po[j] - v0[j] for j in range(3)))
    front = (s < 0) != ((scene.flags[hits["inst"][hit]] & FLIP) != 0)
    kinds[hit] = np.where(front, FRONT, BACK)
    s_out[hit] = s
    return kinds, s_out


def brute32(scene, points, cull_mask=0xFF, cand=None, chunk=1 << 21):
    """HIT_DTYPE records: the smallest key (d2, inst, prim) over the admitted triangles with d2 <= r_max * r_max, t = sqrt(d2); the miss
    record otherwise and for invalid records.  cand: optional list of triangle index arrays per point (candidates())"""
    pts = np.ascontiguousarray(points, F).reshape(-1, 4)
    n = len(pts)
    out = np.zeros(n, HIT_DTYPE)
    out["t"] = pts[:, 3]; out["prim"] = -1; out["inst"] = -1
    with np.errstate(all="ignore"):
        valid = np.isfinite(pts[:, :3]).all(axis=1) & (pts[:, 3] >= 0)
        r2 = pts[:, 3] * pts[:, 3]
    adm = np.nonzero(scene.admitted(cull_mask))[0]

    def resolve(i, tri):
        if len(tri) == 0:
            return
        p = tuple(pts[i, k][:, None] for k in range(3))
        d2, u, v = tri_d2(p, tuple(scene.a[tri, k][None, :] for k in range(3)), tuple(scene.ab[tri, k][None, :] for k in range(3)),
                          tuple(scene.ac[tri, k][None, :] for k in range(3)))
        ok = ~np.isnan(d2) & (d2 <= r2[i][:, None])
        key = np.where(ok, d2, np.inf)
        j = np.argmin(key, axis=1)
        rows = np.arange(len(i))
        bad = ~ok[rows, j]
        j = np.where(bad, np.argmax(ok, axis=1), j)
        got = ok[rows, j]
        ii, jj = i[got], j[got]
        out["t"][ii] = np.sqrt(d2[rows[got], jj]); out["u"][ii] = u[rows[got], jj]; out["v"][ii] = v[rows[got], jj]
        out["prim"][ii] = scene.prim[tri[jj]]; out["inst"][ii] = scene.inst[tri[jj]]

    idx = np.nonzero(valid)[0]
    if cand is None:
        per = max(1, chunk // max(1, len(adm)))
        for k0 in range(0, len(idx), per):
            resolve(idx[k0:k0 + per], adm)
    else:
        for i in idx:
            resolve(np.array([i]), np.asarray(cand[i], np.int64))
    return out


def _segment_d2(p, a, b):
    ab = b - a
    den = (ab * ab).sum(-1)
    t = np.clip(((p - a) * ab).sum(-1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
    q = a + t[..., None] * ab
    return ((p - q) ** 2).sum(-1), q


def _tri_d2_64(p, A, B, C, N, nn):
    """(points, triangles) squared distances and nearest points in binary64"""
    w = p - A
    with np.errstate(all="ignore"):
        u = (np.cross(w, C - A) * N).sum(-1) / nn
        v = (np.cross(B - A, w) * N).sum(-1) / nn
        h = (w * N).sum(-1)
        inside = (nn > 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
        best = np.where(inside, h * h / nn, np.inf)
    q = p - (h / np.where(nn > 0, nn, 1.0))[..., None] * N
    for s0, s1 in ((A, B), (B, C), (C, A)):
        d, qs = _segment_d2(p, s0, s1)
        take = d < best
        best = np.where(take, d, best)
        q = np.where(take[..., None], qs, q)
    return best, q, w


def brute64(scene, points, cull_mask=0xFF, picked=None, chunk=1 << 20):
    """binary64, every admitted triangle as a convex set.  dict: t, inst, prim (nearest; -1 without any triangle), q (the nearest point),
    runner (the distance of the nearest triangle that does NOT touch q — triangles that share the vertex or edge q lies on are at the
    same distance by construction and are no runner-up; inf without one), touching (how many triangles touch q), picked_touches (with
    picked = (inst, prim) arrays: that triangle touches q), side_s / side_scale (s and |n| |p - v0| of triangle `picked`, or of the
    nearest, in binary64 world space), mag (largest coordinate magnitude of the point and the nearest triangle).  r_max is not applied."""
    pts = np.asarray(points, np.float64).reshape(-1, 4)[:, :3]
    n = len(pts)
    adm = np.nonzero(scene.admitted(cull_mask))[0]
    res = dict(t=np.full(n, np.inf), inst=np.full(n, -1, np.int64), prim=np.full(n, -1, np.int64), runner=np.full(n, np.inf),
               q=np.zeros((n, 3)), side_s=np.zeros(n), side_scale=np.zeros(n), mag=np.zeros(n), touching=np.zeros(n, np.int64),
               picked_touches=np.zeros(n, bool))
    if len(adm) == 0:
        return res
    A, B, C = scene.A[adm][None], scene.B[adm][None], scene.C[adm][None]
    N = np.cross(B - A, C - A)
    nn = (N * N).sum(-1)
    first = np.concatenate([[0], np.cumsum(np.bincount(scene.inst, minlength=len(scene.mask)))])
    where = np.full(scene.n_tris, -1, np.int64); where[adm] = np.arange(len(adm))
    per = max(1, chunk // len(adm))
    for k0 in range(0, n, per):
        p = pts[k0:k0 + per][:, None, :]
        best, q, w = _tri_d2_64(p, A, B, C, N, nn)
        rows = np.arange(best.shape[0])
        j = np.argmin(best, axis=1)
        sl = slice(k0, k0 + best.shape[0])
        res["t"][sl] = np.sqrt(best[rows, j])
        res["inst"][sl] = scene.inst[adm[j]]; res["prim"][sl] = scene.prim[adm[j]]
        qj = q[rows, j]
        res["q"][sl] = qj
        tri_mag = np.maximum(np.maximum(np.abs(A[0][j]).max(-1), np.abs(B[0][j]).max(-1)), np.abs(C[0][j]).max(-1))
        mag = np.maximum(np.abs(pts[sl]).max(-1), tri_mag)
        res["mag"][sl] = mag
        dq, _, _ = _tri_d2_64(qj[:, None, :], A, B, C, N, nn)
        # (a packet holds v0 and binary32-rounded edges: the shared vertex of two triangles differs by a few 2^-24 of its magnitude between them)
        touch = np.sqrt(dq) <= 8 * 2.0 ** -24 * mag[:, None]   # (a few binary32 ulps of the magnitude)
        res["touching"][sl] = touch.sum(axis=1)
        res["runner"][sl] = np.sqrt(np.where(touch, np.inf, best).min(axis=1))
        js = j
        if picked is not None:
            pi, pp = np.asarray(picked[0])[sl], np.asarray(picked[1])[sl]
            g = np.where(pi >= 0, where[np.clip(first[np.clip(pi, 0, None)] + pp, 0, scene.n_tris - 1)], -1)
            res["picked_touches"][sl] = np.where(g >= 0, touch[rows, np.clip(g, 0, None)], False)
            js = np.where(g >= 0, g, j)
        Nj, wj = N[0][js], w[rows, js]
        res["side_s"][sl] = (Nj * wj).sum(-1)
        res["side_scale"][sl] = np.sqrt((Nj * Nj).sum(-1)) * np.sqrt((wj * wj).sum(-1))
    return res


def t_tolerance(t, mag):
    """the project's query tolerance (query_reference.t_tolerance's form): 1e-5 of t and 1e-6 of the largest coordinate magnitude"""
    return 1e-5 * np.abs(t) + 1e-6 * mag


def candidates(scene, points, cull_mask=0xFF, chunk=1 << 24):
    """per point the admitted triangles that can hold the smallest key: those whose bounding box is no farther (binary64, 1e-3 relative
    and 1e-4 of the magnitudes as margin) than the smallest farthest-corner distance of any box.  Runs on the GPU through torch when one is there."""
    pts = np.asarray(points, np.float64).reshape(-1, 4)[:, :3]
    adm = np.nonzero(scene.admitted(cull_mask))[0]
    lo = np.minimum(np.minimum(scene.A[adm], scene.B[adm]), scene.C[adm])
    hi = np.maximum(np.maximum(scene.A[adm], scene.B[adm]), scene.C[adm])
    try:
        import torch
        use = torch.cuda.is_available()
    except ImportError:
        use = False
    out = [np.zeros(0, np.int64)] * len(pts)
    if len(adm) == 0:
        return out
    per = max(1, chunk // len(adm))
    if use:
        tlo, thi = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
    for k0 in range(0, len(pts), per):
        p = pts[k0:k0 + per]
        if use:
            tp = torch.from_numpy(p).cuda()[:, None, :]
            near = torch.clamp(torch.maximum(tlo[None] - tp, tp - thi[None]), min=0.0).pow(2).sum(-1).sqrt()
            far = torch.maximum((tp - tlo[None]).abs(), (tp - thi[None]).abs()).pow(2).sum(-1).sqrt()
            near, far = near.cpu().numpy(), far.cpu().numpy()
        else:
            q = p[:, None, :]
            near = np.sqrt((np.maximum(np.maximum(lo[None] - q, q - hi[None]), 0.0) ** 2).sum(-1))
            far = np.sqrt((np.maximum(np.abs(q - lo[None]), np.abs(q - hi[None])) ** 2).sum(-1))
        mag = np.maximum(np.abs(p).max(-1), max(np.abs(lo).max(), np.abs(hi).max()))
        ub = np.where(np.isfinite(p).all(-1), far.min(axis=1) * (1 + 1e-3) + 1e-4 * mag, np.inf)
        keep = near <= ub[:, None]
        for r in range(len(p)):
            out[k0 + r] = adm[np.nonzero(keep[r])[0]]
    return out
