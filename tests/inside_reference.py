"""References for rt_point_inside_device (include/rt_api.h; DESIGN.md §5 "Inside / outside"), none with a tree:

 * words(): the vote over the crossing parities restated from the header's text;
 * oracle_counts(): count_k(p) from the oracle's query_candidate over every triangle of the scene, for the rays compose_rays() builds
   (the rays a torch user would hand to rt_intersect_device_hits);
 * winding(): the binary64 winding number of the scene about a point, summed over the instances as absolute values (a mirrored
   instance winds the other way), the truth the vote's bit is held to.

inside_scene() and adversarial_points() are the experiment that chose three directions: closed meshes under rotated, sheared and
mirrored instances, and points from which the ray along one of the first three table directions passes through a vertex or an edge."""
import numpy as np

from tests.test_ray_query_oracle import oracle_scene, placed_instances, small_meshes
from vulkan_raytracing_amd import api

DIRS = np.array(api.INSIDE_DIRS, np.float32)
INF = np.float32(np.inf)


def words(counts, n_dirs, all_dirs):
    """the vote word of every row of counts (n, >= n_dirs): directions in order, stop once odd or even holds more than n_dirs // 2 votes
    (all_dirs: never); bit 0 odd won, bits 8-15 the odd votes among the directions taken, bits 16-23 the directions taken"""
    counts = np.asarray(counts, np.uint32).reshape(len(counts), -1)
    half = n_dirs // 2
    odd = np.cumsum(counts[:, :n_dirs] & 1, axis=1).astype(np.uint32)           # odd votes after 1, 2, ... directions
    even = np.arange(1, n_dirs + 1, dtype=np.uint32)[None, :] - odd
    decided = (odd > half) | (even > half)                                       # (true in the last column: n_dirs is odd)
    taken = np.full(len(counts), n_dirs, np.uint32) if all_dirs else (np.argmax(decided, axis=1) + 1).astype(np.uint32)
    votes = odd[np.arange(len(counts)), taken - 1] if len(counts) else np.zeros(0, np.uint32)
    return (votes > half).astype(np.uint32) | (votes << 8) | (taken << 16)


def compose_rays(points, n_dirs):
    """(n * n_dirs, 8) float32, point-major: (p, tmin 0, D_k, tmax +inf)"""
    p = np.asarray(points, np.float32).reshape(len(points), -1)[:, :3]
    r = np.zeros((len(p), n_dirs, 8), np.float32)
    r[:, :, 0:3] = p[:, None, :]
    r[:, :, 4:7] = DIRS[None, :n_dirs, :]
    r[:, :, 7] = INF
    return r.reshape(-1, 8)


def tri_counts(ranges, inst):
    return np.array([ranges[int(r["mesh"])][2] for r in inst], np.int64)


def oracle_counts(orc, tc, points, n_dirs, cull=0xFF, chunk=1 << 20):
    """(n, n_dirs) uint32: the candidates OracleScene.query_candidate accepts over every (inst, prim) for the composed rays, ray flags 0"""
    rays = compose_rays(points, n_dirs)
    n = len(rays)
    inst_ids = np.repeat(np.arange(len(tc), dtype=np.int32), tc)
    prim_ids = np.concatenate([np.arange(c, dtype=np.int32) for c in tc])
    T = len(inst_ids)
    per = max(1, chunk // T)
    counts = np.zeros(n, np.int64)
    for r0 in range(0, n, per):
        r1 = min(n, r0 + per)
        ok = orc.query_candidate(np.repeat(rays[r0:r1], T, axis=0), np.tile(inst_ids, r1 - r0), np.tile(prim_ids, r1 - r0), None, 0, cull)[0]
        counts[r0:r1] = ok.reshape(r1 - r0, T).sum(axis=1)
    return counts.astype(np.uint32).reshape(-1, n_dirs)


# ---- the scene of the experiment ----------------------------------------------------------------------------------------------

def closed_meshes():
    """mesh 0: small_meshes' octahedron, mesh 1: the cube [-1, 1]^3 (12 triangles), mesh 2: a 12 x 8 torus (R 1, r 0.4); all closed and
    consistently wound"""
    v, ix, _ = small_meshes()
    octa = np.asarray(v, np.float32).reshape(-1, 6)[:6, :3]
    octa_idx = np.asarray(ix[:24], np.uint32)
    cube = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    cube_idx = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32).reshape(-1)
    nu, nv = 12, 8
    a = 2 * np.pi * np.arange(nu) / nu
    b = 2 * np.pi * np.arange(nv) / nv
    A, B = np.meshgrid(a, b, indexing="ij")
    torus = np.stack([(1 + 0.4 * np.cos(B)) * np.cos(A), (1 + 0.4 * np.cos(B)) * np.sin(A), 0.4 * np.sin(B)], axis=-1).reshape(-1, 3).astype(np.float32)
    tt = []
    for i in range(nu):
        for j in range(nv):
            p00, p10, p11, p01 = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            tt += [(p00, p10, p11), (p00, p11, p01)]
    torus_idx = np.array(tt, np.uint32).reshape(-1)
    pos = np.concatenate([octa, cube, torus])
    nrm = pos / np.maximum(np.linalg.norm(pos, axis=1, keepdims=True), 1e-6)
    verts = np.concatenate([pos, nrm], axis=1).astype(np.float32).reshape(-1)
    idx = np.concatenate([octa_idx, cube_idx, torus_idx])
    ranges = [(0, 0, 8), (6 * 6, 24, 12), (6 * 14, 24 + 36, 2 * nu * nv)]
    return verts, idx, ranges


def inside_scene(seed=301):
    """closed_meshes under 12 instances of placed_instances (rotated, scaled, sheared, mirrored), every mask 0xFF"""
    verts, idx, ranges = closed_meshes()
    inst = placed_instances(12, seed, spacing=4.0, mesh_scale=(1.0, 1.0, 1.0), n_meshes=3)
    inst["custom_index_and_mask"] |= np.uint32(0xFF000000)
    return verts, idx, ranges, inst


def mesh_triangles(verts, idx, ranges, mesh):
    """(T, 3, 3) float64 object-space vertices of a mesh's triangles"""
    ff, fi, pc = ranges[mesh]
    p = np.asarray(verts, np.float32)[ff:].reshape(-1, 6)[:, :3].astype(np.float64)
    return p[np.asarray(idx[fi:fi + 3 * pc], np.int64).reshape(-1, 3)]


def adversarial_points(parts, seed=302):
    """(points float32 (n, 4) with w = +inf, adversarial bool (n,)): per instance 300 random points of [-1.6, 1.6]^3 in object space,
    and, for each of D0..D2, vertex - s D_k (s in 0.3, 0.9, 2.5) and edge point - s D_k (s in 0.25, 1.7) at the midpoint and one random
    point of every edge of every triangle; the offsets are taken in world space, so the ray along D_k runs through the feature"""
    verts, idx, ranges, inst = parts
    rng = np.random.default_rng(seed)
    D = DIRS[:3].astype(np.float64)
    pts, adv = [], []
    for r in inst:
        M = np.asarray(r["transform"], np.float64).reshape(3, 4)
        to_world = lambda p: p @ M[:, :3].T + M[:, 3]   # noqa: E731
        tri = mesh_triangles(verts, idx, ranges, int(r["mesh"]))
        pts.append(to_world(rng.uniform(-1.6, 1.6, (300, 3)))); adv.append(np.zeros(300, bool))
        vtx = to_world(np.unique(tri.reshape(-1, 3), axis=0))
        e0 = to_world(tri.reshape(-1, 3))
        e1 = to_world(tri[:, [1, 2, 0], :].reshape(-1, 3))
        t = rng.uniform(size=(len(e0), 1))
        on_edge = np.concatenate([(e0 + e1) / 2, e0 + t * (e1 - e0)])
        for k in range(3):
            for s in (0.3, 0.9, 2.5):
                pts.append(vtx - s * D[k]); adv.append(np.ones(len(vtx), bool))
            for s in (0.25, 1.7):
                pts.append(on_edge - s * D[k]); adv.append(np.ones(len(on_edge), bool))
    p = np.concatenate(pts).astype(np.float32)
    return np.concatenate([p, np.full((len(p), 1), np.inf, np.float32)], axis=1), np.concatenate(adv)


def winding(parts, points, chunk=4096):
    """the binary64 winding number of the scene about every point: per instance |sum of the triangles' signed solid angles| / 4 pi
    (van Oosterom and Strackee), summed over the instances"""
    verts, idx, ranges, inst = parts
    p = np.asarray(points, np.float32).reshape(len(points), -1)[:, :3].astype(np.float64)
    total = np.zeros(len(p))
    for r in inst:
        M = np.asarray(r["transform"], np.float32).astype(np.float64).reshape(3, 4)
        tri = mesh_triangles(verts, idx, ranges, int(r["mesh"])) @ M[:, :3].T + M[:, 3]
        T = [[tri[None, :, k, j] for j in range(3)] for k in range(3)]
        for c0 in range(0, len(p), chunk):
            q = p[c0:c0 + chunk]
            (ax, ay, az), (bx, by, bz), (cx, cy, cz) = ([T[k][j] - q[:, j:j + 1] for j in range(3)] for k in range(3))
            la, lb, lc = np.sqrt(ax * ax + ay * ay + az * az), np.sqrt(bx * bx + by * by + bz * bz), np.sqrt(cx * cx + cy * cy + cz * cz)
            num = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
            den = la * lb * lc + (ax * bx + ay * by + az * bz) * lc + (bx * cx + by * cy + bz * cz) * la + (cx * ax + cy * ay + cz * az) * lb
            total[c0:c0 + chunk] += np.abs((2.0 * np.arctan2(num, den)).sum(axis=1)) / (4 * np.pi)
    return total


_CACHE = {}


def experiment():
    """the scene, its oracle, the points and everything the CPU and GPU tests share, computed once: dict of parts, orc, tc, points, adv,
    counts (n, 5), wind (n,), kept (n,) bool (winding within 0.05 of an integer), truth (n,) uint32 (its parity)"""
    if "experiment" not in _CACHE:
        parts = inside_scene()
        verts, idx, ranges, inst = parts
        orc = oracle_scene(verts, idx, ranges, inst)
        tc = tri_counts(ranges, inst)
        points, adv = adversarial_points(parts)
        counts = oracle_counts(orc, tc, points, 5)
        wind = winding(parts, points)
        near = np.rint(wind)
        _CACHE["experiment"] = dict(parts=parts, orc=orc, tc=tc, points=points, adv=adv, counts=counts, wind=wind,
                                    kept=np.abs(wind - near) <= 0.05, truth=near.astype(np.int64).astype(np.uint32) & 1)
    return _CACHE["experiment"]
