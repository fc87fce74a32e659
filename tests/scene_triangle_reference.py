"""The reference for rt_scene_triangles_device, rt_overlap_scene_triangles_device and rt_closest_scene_triangle_device (include/rt_api.h;
DESIGN.md §5 "Triangles of the scene as the query"), without a tree:

 * expand: the 48-byte record of every (inst, prim, against, r_max) reference from closest_reference.Scene's canonical transforms
   (a, a + ab, a + ac in binary32), nine quiet NaNs for an invalid reference;
 * overlaps: triangle_overlap_reference's surviving pairs and canonical predicate over those records, the instance rule in front of
   overlap_reference.rows;
 * nearest: triangle_distance_reference.tri_tri32 over those records, the instance rule in front of the key's minimum.

The instance rule removes pairs; it never changes the test of a pair that stays."""
import numpy as np

from tests import overlap_reference as orf
from tests import triangle_distance_reference as tdr
from tests import triangle_overlap_reference as trf
from tests.closest_reference import F
from vulkan_raytracing_amd.api import HIT_DTYPE

QNAN = np.uint32(0x7FC00000)
BAD_LIMIT = F(1e37)


def refs(inst, prim, against=-1, r_max=np.inf):
    """(n, 4) int32 rows; api.triangle_refs restated (the reference does not lean on the code under test)"""
    i, p, a, r = np.broadcast_arrays(*(np.asarray(x).reshape(-1) for x in (inst, prim, against, r_max)))
    out = np.zeros((len(i), 4), np.int32)
    out[:, 0] = i; out[:, 1] = p; out[:, 2] = a
    out[:, 3] = np.ascontiguousarray(r, F).view(np.int32)
    return out


def every_triangle(scene, against=-1, r_max=np.inf):
    """one reference per triangle of the scene, in (inst, prim) order"""
    return refs(scene.inst, scene.prim, against, r_max)


class Source:
    """what a reference may name: per instance the first triangle in closest_reference.Scene's arrays and the triangle count of its mesh,
    and per triangle whether it is a BAD TRIANGLE (an object-space coordinate that is not finite or of magnitude >= 1e37)"""

    def __init__(self, scene, verts6, idx, ranges, instances):
        self.scene = scene
        self.n_inst = len(instances)
        self.count = np.array([ranges[int(r["mesh"])][2] for r in instances], np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.count)])[:-1]
        verts = np.asarray(verts6, F).reshape(-1)
        bad = []
        for r in instances:
            ff, fi, pc = ranges[int(r["mesh"])]
            ix = np.asarray(idx, np.int64)[fi:fi + 3 * pc].reshape(-1, 3)
            p = verts[ff:].reshape(-1, 6)[:, :3][ix].reshape(-1, 9)
            with np.errstate(invalid="ignore"):
                bad.append(~(np.isfinite(p).all(axis=1) & (np.abs(p) < BAD_LIMIT).all(axis=1)))
        self.bad = np.concatenate(bad) if bad else np.zeros(0, bool)
        self.tris = trf.Triangles(scene)


def expand(src, r):
    """(records (n, 12) float32, valid (n,) bool, triangle (n,) index into the Scene's arrays or -1)"""
    r = np.asarray(r, np.int32).reshape(-1, 4)
    inst, prim, against = r[:, 0].astype(np.int64), r[:, 1].astype(np.int64), r[:, 2].astype(np.int64)
    ok = (inst >= 0) & (inst < src.n_inst) & (against >= -1) & (against < src.n_inst)
    ok &= (prim >= 0) & (prim < src.count[np.clip(inst, 0, src.n_inst - 1)])
    tri = np.where(ok, src.first[np.clip(inst, 0, src.n_inst - 1)] + prim, -1)
    t = src.tris
    k = np.clip(tri, 0, None)
    ok &= ~src.bad[k] & t.finite[k]
    out = np.zeros((len(r), 12), np.uint32)
    out[:, trf.COLS] = QNAN
    P = np.concatenate([t.A[k], t.B[k], t.C[k]], axis=1).view(np.uint32)
    cols = np.array(trf.COLS)
    out[np.ix_(ok, cols)] = P[ok]
    out[:, 3] = r[:, 3].view(np.uint32); out[:, 7] = r[:, 0].view(np.uint32); out[:, 11] = r[:, 2].view(np.uint32)
    return out.view(F), ok, np.where(ok, tri, -1)


def allowed(src, r, ti, qi=None):
    """the instance rule for the pairs (reference qi[k], scene triangle ti[k]) (qi None: every reference against every ti, (n, m))"""
    r = np.asarray(r, np.int32).reshape(-1, 4)
    cand = src.scene.inst[ti].astype(np.int64)
    if qi is None:
        inst, against = r[:, 0:1].astype(np.int64), r[:, 2:3].astype(np.int64)
        cand = cand[None, :]
    else:
        inst, against = r[qi, 0].astype(np.int64), r[qi, 2].astype(np.int64)
    return np.where(against < 0, cand != inst, cand == against)


def overlaps(src, r, cull_mask=0xFF, max_ids=16, rule=True):
    """counts (n,) uint32 and ids (n, max_ids, 2) int32; rule=False: the plain call over the expanded records"""
    q, ok, _ = expand(src, r)
    qi, ti = trf.surviving_pairs(src.tris, q, cull_mask)
    keep = trf.candidates32(src.tris, q, qi, ti)
    if rule:
        keep &= allowed(src, r, ti, qi)
    return orf.rows(src.scene, len(q), qi, ti, keep, max_ids)


def nearest(src, r, cull_mask=0xFF, rule=True, chunk=1 << 18):
    """(HIT_DTYPE records, (n, 2) float32 (qu, qv)): triangle_distance_reference.brute32 over the expanded records with the instance rule
    in front of the key's minimum"""
    scene = src.scene
    tr, _, _ = expand(src, r)
    n = len(tr)
    out = np.zeros(n, HIT_DTYPE)
    out["t"] = tr[:, 3]; out["prim"] = -1; out["inst"] = -1
    quv = np.zeros((n, 2), F)
    with np.errstate(all="ignore"):
        r2 = tr[:, 3] * tr[:, 3]
    tri = np.nonzero(scene.admitted(cull_mask))[0]
    idx = np.nonzero(tdr.valid_triangles(tr))[0]
    if len(tri) == 0:
        return out, quv
    per = max(1, chunk // len(tri))
    ta, tab, tac = (tuple(getattr(scene, name)[tri, k][None, :] for k in range(3)) for name in ("a", "ab", "ac"))
    for k0 in range(0, len(idx), per):
        i = idx[k0:k0 + per]
        P = tuple(tuple(tr[i, 4 * v + k][:, None] for k in range(3)) for v in range(3))
        d2, u, v, qu, qv = tdr.tri_tri32(P, ta, tab, tac)
        with np.errstate(invalid="ignore"):
            ok = ~np.isnan(d2) & (d2 <= r2[i][:, None])
        if rule:
            ok &= allowed(src, np.asarray(r, np.int32).reshape(-1, 4)[i], tri)
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
    return out, quv
