"""An independent binary64 restatement of rt_intersect_device_flags' rules (include/rt_api.h; Vulkan's ray-traversal chapter) for small
scenes: every ray against every world triangle, no tree, no oracle.  It is the second implementation the oracle's orc_intersect_query and
the GPU are compared with.

Binary64 and binary32 can disagree only near a decision boundary, so the reference reports a ray as AMBIGUOUS when a candidate that could
matter (a triangle of an instance the ray enters, within the tolerance of the ray's interval and of the triangle) lies within a relative
REL of a triangle edge (a barycentric near 0), of det = 0 (|det| / (|e1| |e2| |d|)), of tmin or tmax, or when the two nearest surviving
candidates lie within REL of each other in t.  Rays with non-finite components or a zero direction are ambiguous too.  Everything else
must agree with binary32 implementations exactly in (inst, prim, kind), and in t to 1e-5 relative, or to the bound t_tolerance() gives a
hit that is nearly parallel to its triangle (the binary32 error of t grows like 1 / |det|)."""
import numpy as np

REL = 1e-4
OPAQUE, NO_OPAQUE, TERMINATE = 0x1, 0x2, 0x4
CULL_BACK, CULL_FRONT, CULL_OPAQUE, CULL_NO_OPAQUE, SKIP_TRIANGLES = 0x10, 0x20, 0x40, 0x80, 0x100
FCD, FLIP, FORCE_OPAQUE, FORCE_NO_OPAQUE = 0x1, 0x2, 0x4, 0x8
FRONT, BACK = 0xFE, 0xFF


class Scene:
    """instances (INSTANCE_DTYPE records) over meshes given as (verts6, idx, ranges) in the upload layout"""

    def __init__(self, verts6, idx, ranges, instances):
        verts = np.asarray(verts6, np.float32).reshape(-1)
        idx = np.asarray(idx, np.int64)
        self.meshes = []
        for ff, fi, pc in ranges:
            ix = idx[fi:fi + 3 * pc].reshape(-1, 3)
            p = verts[ff:].reshape(-1, 6)[:, :3].astype(np.float64)
            v0, v1, v2 = p[ix[:, 0]], p[ix[:, 1]], p[ix[:, 2]]
            self.meshes.append((v0, v1 - v0, v2 - v0))
        self.inst = []
        for r in instances:
            M = np.asarray(r["transform"], np.float64).reshape(3, 4)
            self.inst.append(dict(A=np.linalg.inv(M[:, :3]), t=M[:, 3], mask=int(r["custom_index_and_mask"]) >> 24,
                                  flags=(int(r["sbt_offset_and_flags"]) >> 24) & 0xFF, mesh=int(r["mesh"])))
        self.offset = np.cumsum([0] + [len(self.meshes[i["mesh"]][0]) for i in self.inst])


def _visible(flags, cull, inst):
    """(R,) bool: the rays enter the instance (cull mask, opacity, SkipTriangles)"""
    f = inst["flags"]
    opaque = np.where(flags & OPAQUE, True, np.where(flags & NO_OPAQUE, False, True if f & FORCE_OPAQUE else not (f & FORCE_NO_OPAQUE)))
    skip = ((flags & SKIP_TRIANGLES) != 0) | (opaque & ((flags & CULL_OPAQUE) != 0)) | (~opaque & ((flags & CULL_NO_OPAQUE) != 0))
    return ((inst["mask"] & cull) != 0) & ~skip


def query(scene, rays, words=None, ray_flags=0, cull_mask=0xFF, chunk=2048):
    """the rules for every ray: dict of inst, prim, t, u, v, kind (closest surviving candidate; -1 / 0 on a miss), blocked (any survivor),
    ambiguous, and survivors: (n, world triangles) bool, world triangle k = scene.offset[inst] + prim"""
    rays = np.asarray(rays, np.float32).reshape(-1, 8)
    n = len(rays)
    w = np.full(n, 0xFF000000, np.uint64) if words is None else np.asarray(words, np.uint32).astype(np.uint64)
    flags = (int(ray_flags) | (w & 0x3FF)).astype(np.int64)
    cull = (int(cull_mask) & (w >> 24)).astype(np.int64)
    n_tri = int(scene.offset[-1])
    out = dict(inst=np.full(n, -1, np.int32), prim=np.full(n, -1, np.int32), t=np.zeros(n), u=np.zeros(n), v=np.zeros(n),
               kind=np.zeros(n, np.uint32), rel_det=np.ones(n), blocked=np.zeros(n, bool), ambiguous=np.zeros(n, bool), survivors=np.zeros((n, n_tri), bool))
    for c0 in range(0, n, chunk):
        sl = slice(c0, min(n, c0 + chunk))
        r = rays[sl].astype(np.float64)
        O, D, tmin, tmax = r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7]
        fl, cm = flags[sl], cull[sl]
        amb = ~np.isfinite(r).all(axis=1) | (np.abs(D).sum(axis=1) == 0) | ~(tmin < tmax)
        T, U, V, K, RD = [], [], [], [], []
        surv = []
        with np.errstate(all="ignore"):
            for inst in scene.inst:
                v0, e1, e2 = scene.meshes[inst["mesh"]]
                vis = _visible(fl, cm, inst)
                oo = (O - inst["t"]) @ inst["A"].T
                od = D @ inst["A"].T
                p = np.cross(od[:, None, :], e2[None, :, :])
                det = np.einsum("tk,rtk->rt", e1, p)
                s = oo[:, None, :] - v0[None, :, :]
                u = np.einsum("rtk,rtk->rt", s, p) / det
                q = np.cross(s, e1[None, :, :])
                v = np.einsum("rk,rtk->rt", od, q) / det
                t = np.einsum("tk,rtk->rt", e2, q) / det
                scale = np.linalg.norm(e1, axis=1)[None, :] * np.linalg.norm(e2, axis=1)[None, :] * np.linalg.norm(od, axis=1)[:, None]
                rel_det = np.abs(det) / scale
                tm, tM = tmin[:, None], tmax[:, None]
                near = (u >= -REL) & (v >= -REL) & (u + v <= 1 + REL) & (t > tm - REL * np.abs(tm)) & (t < tM + REL * np.abs(tM)) & vis[:, None]
                near |= vis[:, None] & (rel_det < REL) & np.isfinite(rel_det)   # a grazing triangle: barycentrics say nothing
                close = ((np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(1 - u - v)) < REL) | ~(rel_det >= REL)
                         | (np.abs(t - tm) <= REL * np.maximum(np.abs(t), np.abs(tm))) | (np.abs(t - tM) <= REL * np.maximum(np.abs(t), np.abs(tM))))
                amb |= (near & close).any(axis=1)
                front = (det < 0) != bool(inst["flags"] & FLIP)
                culled = np.zeros_like(front) if inst["flags"] & FCD else ((front & ((fl & CULL_FRONT) != 0)[:, None]) | (~front & ((fl & CULL_BACK) != 0)[:, None]))
                ok = vis[:, None] & ~culled & (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tm) & (t < tM)
                surv.append(ok)
                T.append(np.where(ok, t, np.inf)); U.append(u); V.append(v); K.append(np.where(front, FRONT, BACK)); RD.append(rel_det)
        # (a candidate near the boundary of the surviving set is already ambiguous above: the tie check needs the survivors only)
        T, U, V, K, S, RD = (np.concatenate(x, axis=1) for x in (T, U, V, K, surv, RD))
        k = np.argmin(T, axis=1)   # first minimum: the smallest (instance, prim) of equal t, as the tie rule
        rows = np.arange(len(k))
        hit = np.isfinite(T[rows, k])
        srt = np.sort(T, axis=1)
        if srt.shape[1] > 1:
            t0, t1 = srt[:, 0], srt[:, 1]
            with np.errstate(invalid="ignore"):   # (inf - inf: no second survivor)
                amb |= np.isfinite(t1) & (np.abs(t1 - t0) <= REL * np.maximum(np.abs(t0), np.abs(t1)))
        ii = np.searchsorted(scene.offset, k, side="right") - 1
        out["inst"][sl] = np.where(hit, ii, -1)
        out["prim"][sl] = np.where(hit, k - scene.offset[ii], -1)
        out["t"][sl] = np.where(hit, T[rows, k], tmax)
        out["u"][sl] = np.where(hit, U[rows, k], 0)
        out["v"][sl] = np.where(hit, V[rows, k], 0)
        out["kind"][sl] = np.where(hit, K[rows, k], 0)
        out["rel_det"][sl] = np.where(hit, RD[rows, k], 1.0)
        out["blocked"][sl] = hit
        out["ambiguous"][sl] = amb
        out["survivors"][sl] = S
    return out


def t_tolerance(res, rays):
    """absolute tolerance of a binary32 t against the reference's: 1e-5 of t, widened to 1e-6 / (|det| / (|e1| |e2| |d|)) of t for grazing
    hits, and at least 1e-6 of the origin's distance from the world origin (the binary32 object-space origin is rounded at that scale)"""
    rays = np.asarray(rays, np.float64).reshape(-1, 8)
    rel = np.maximum(1e-5, 1e-6 / np.maximum(res["rel_det"], 1e-300))
    return np.maximum(rel * np.abs(res["t"]), 1e-6 * np.linalg.norm(rays[:, 0:3], axis=1) / np.maximum(np.linalg.norm(rays[:, 4:7], axis=1), 1e-30))
