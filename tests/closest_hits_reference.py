"""The reference of rt_closest_point_device_hits (include/rt_api.h; DESIGN.md §5 "K nearest triangles"), without a tree: brute32_k, the
canonical binary32 d2 of tests/closest_reference.py (tri_d2 over closest_reference.Scene) of every admitted triangle, the candidates
(d2 not NaN, d2 <= r_max * r_max) sorted by the key (d2, inst, prim), the first max_hits of them per point and their uncapped number.
The GPU is held to it byte for byte."""
import numpy as np

from tests import closest_reference as cr
from vulkan_raytracing_amd.api import HIT_DTYPE

F = np.float32


def all_d2(scene, points, cull_mask=0xFF):
    """(admitted triangle indices, d2, u, v as (points, admitted) binary32 arrays): the canonical test of every admitted triangle"""
    pts = np.ascontiguousarray(points, F).reshape(-1, 4)
    adm = np.nonzero(scene.admitted(cull_mask))[0]
    p = tuple(pts[:, k][:, None] for k in range(3))
    d2, u, v = cr.tri_d2(p, tuple(scene.a[adm, k][None, :] for k in range(3)), tuple(scene.ab[adm, k][None, :] for k in range(3)),
                         tuple(scene.ac[adm, k][None, :] for k in range(3)))
    shape = (len(pts), len(adm))
    return adm, np.broadcast_to(d2, shape), np.broadcast_to(u, shape), np.broadcast_to(v, shape)


def brute32_k(scene, points, max_hits, cull_mask=0xFF, chunk=1 << 21):
    """(HIT_DTYPE (n, max_hits), uint32 (n,)): per point the max_hits smallest candidates by (d2, inst, prim) with t = sqrt(d2) in
    binary32, the miss form (t = r_max as given, u = v = 0, prim = inst = -1) behind them, and the number of candidates, not capped.
    Invalid records (a non-finite coordinate, a negative or NaN r_max): miss rows and a count of 0."""
    pts = np.ascontiguousarray(points, F).reshape(-1, 4)
    n, K = len(pts), int(max_hits)
    hits = np.zeros((n, K), HIT_DTYPE)
    hits["t"] = pts[:, 3][:, None]; hits["prim"] = -1; hits["inst"] = -1
    counts = np.zeros(n, np.uint32)
    with np.errstate(all="ignore"):
        valid = np.isfinite(pts[:, :3]).all(axis=1) & (pts[:, 3] >= 0)
        r2 = pts[:, 3] * pts[:, 3]
    idx = np.nonzero(valid)[0]
    per = max(1, chunk // max(1, int(scene.admitted(cull_mask).sum())))
    for k0 in range(0, len(idx), per):
        i = idx[k0:k0 + per]
        adm, d2, u, v = all_d2(scene, pts[i], cull_mask)
        if len(adm) == 0:
            break
        ok = ~np.isnan(d2) & (d2 <= r2[i][:, None])
        row, col = np.nonzero(ok)
        tri = adm[col]
        order = np.lexsort((scene.prim[tri], scene.inst[tri], d2[row, col], row))
        row, col, tri = row[order], col[order], tri[order]
        c = np.bincount(row, minlength=len(i))
        counts[i] = c
        pos = np.arange(len(row)) - np.concatenate([[0], np.cumsum(c)])[row]
        sel = pos < K
        row, col, tri, pos = row[sel], col[sel], tri[sel], pos[sel]
        rec = np.zeros(len(row), HIT_DTYPE)
        rec["t"] = np.sqrt(d2[row, col]); rec["u"] = u[row, col]; rec["v"] = v[row, col]
        rec["prim"] = scene.prim[tri]; rec["inst"] = scene.inst[tri]
        hits[i[row], pos] = rec
    return hits, counts
