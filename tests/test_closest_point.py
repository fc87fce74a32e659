"""rt_closest_point_device / rt_closest_point: the nearest surface point of every query point.

tests/closest_reference.py holds the two references: brute32, the canonical binary32 arithmetic and key of include/rt_api.h and DESIGN.md
§5 restated in numpy over every triangle, and brute64, an independent binary64 minimum over each triangle as a convex set.  The CPU part
holds brute32 to brute64; the GPU part holds the library to brute32 byte for byte: hits, attributes (against the oracle's hit_attributes
of the returned records) and side words, under every tree the library can build, far from the origin, on degenerate geometry, on the cfg3
scene, and the plumbing of a device query.

Identity against binary64: triangles that share the vertex or edge the nearest point lies on are at the same distance by construction
(from outside a convex mesh the nearest point is a vertex or an edge for a large share of space), and which of them binary32 reports is
decided by the key on rounding noise.  So the binary32 triangle must TOUCH the binary64 nearest point, must BE the binary64 triangle
where only one touches it, and only a runner-up that does not touch it and lies within REL excuses a point."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import closest_reference as cr
from tests import scenes
from tests.query_reference import REL
from tests.test_ray_query import PATHS, dev_inst, slow_queue
from tests.test_ray_query_oracle import edge_geometry, edge_instances, oracle_scene, placed_instances, small_meshes, use_builder
from vulkan_raytracing_amd import RtContext, api, host, workloads
from vulkan_raytracing_amd.api import HIT_DTYPE, RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
INF = np.float32(np.inf)


# ---- scenes and point sets ----------------------------------------------------------------------------------------------------

def small_scene(seed=5, n=32, offset=0.0):
    """small_meshes (an octahedron, a soup of 12 triangles) under placed_instances (rigid-and-scaled, sheared, mirrored; eight masks);
    every fourth instance rigid, every eighth uniformly scaled; the whole scene translated by `offset` along (1, 1, 1)"""
    verts, idx, ranges = small_meshes(seed)
    inst = placed_instances(n, seed + 1, spacing=3.0)
    rng = np.random.default_rng(seed + 2)
    for i in range(0, n, 4):
        M = np.asarray(inst[i]["transform"], np.float64).reshape(3, 4)
        U, _, Vt = np.linalg.svd(M[:, :3])
        M[:, :3] = (U @ Vt) * (rng.uniform(0.5, 2.0) if i % 8 else 1.0)
        inst[i]["transform"] = M.astype(np.float32).reshape(12)
    if offset:
        inst["transform"][:, [3, 7, 11]] += np.float32(offset)
    return verts, idx, ranges, inst


def scene_box(sc):
    P = np.concatenate([sc.A, sc.B, sc.C])
    return P.min(axis=0), P.max(axis=0)


def surface_points(sc, n, rng, disp):
    """uniform barycentric samples of random triangles, displaced by up to `disp` along a random direction"""
    k = rng.integers(0, sc.n_tris, n)
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    fl = u + v > 1
    u, v = np.where(fl, 1 - u, u), np.where(fl, 1 - v, v)
    q = sc.A[k] + u[:, None] * (sc.B[k] - sc.A[k]) + v[:, None] * (sc.C[k] - sc.A[k])
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return q + d * rng.uniform(0, disp, (n, 1))


def with_radius(p, r):
    return np.concatenate([np.asarray(p, np.float64), np.broadcast_to(np.asarray(r, np.float64), (len(p),))[:, None]], axis=1).astype(np.float32)


def point_sets(sc, n, seed):
    """near the surface, in the volume (uniform in the scene's box), 50 diagonals away; r_max = inf"""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(sc)
    c, diag = (lo + hi) / 2, np.linalg.norm(hi - lo)
    far = rng.normal(size=(n, 3)); far /= np.linalg.norm(far, axis=1, keepdims=True)
    return {"near": with_radius(surface_points(sc, n, rng, 0.01 * diag), np.inf),
            "volume": with_radius(c + rng.uniform(-0.5, 0.5, (n, 3)) * (hi - lo), np.inf),
            "far": with_radius(c + far * 50 * diag, np.inf)}


def feature_points(sc, n, seed):
    """exactly on world vertices and (to binary32 rounding) on edges"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, sc.n_tris, n)
    on_v = np.where((k % 3 == 0)[:, None], sc.A[k], np.where((k % 3 == 1)[:, None], sc.B[k], sc.C[k]))
    s = rng.uniform(size=(n, 1))
    return with_radius(np.concatenate([on_v, sc.A[k] + s * (sc.B[k] - sc.A[k]), sc.B[k] + s * (sc.C[k] - sc.B[k])]), np.inf)


def invalid_records(p):
    """records the contract answers with the miss form: NaN / inf coordinates, negative and NaN r_max"""
    q = np.array(p[:12], np.float32).copy()
    q[0, 0] = np.nan; q[1, 1] = np.inf; q[2, 2] = -np.inf; q[3, 3] = -1.0; q[4, 3] = np.nan; q[5, 3] = -np.inf
    q[6, 3] = np.float32(-0.0); q[7, 3] = 0.0; q[8, 3] = 3e38; q[9, 3] = 1e-30
    return q


def dev(p):
    import torch
    return torch.from_numpy(np.ascontiguousarray(p, np.float32).reshape(-1, 4)).to("cuda:0")


def gpu_closest(ctx, pts, cull=0xFF, attributes=True):
    import torch
    res = ctx.closest_point_device(dev(pts), cull_mask=cull, attributes=attributes)
    torch.cuda.synchronize()
    return res.numpy()


def check(sc, orc, pts, got, cull=0xFF, what="", cand=None):
    """the GPU's (hits, attributes) against brute32 byte for byte; attributes against orc.hit_attributes of the returned records and the
    restated side words"""
    h, a = got
    ref = cr.brute32(sc, pts, cull, cand=cand)
    if h.tobytes() != ref.tobytes():
        bad = np.nonzero((h.view(np.uint8).reshape(len(h), -1) != ref.view(np.uint8).reshape(len(h), -1)).any(axis=1))[0]
        raise AssertionError("%s: %d records differ from the brute force, first %d: point %s gpu %s reference %s" %
                             (what, len(bad), bad[0], np.asarray(pts).reshape(-1, 4)[bad[0]], h[bad[0]], ref[bad[0]]))
    with np.errstate(invalid="ignore"):
        t = h["t"]
        assert not np.isnan(t[~np.isnan(np.asarray(pts, np.float32).reshape(-1, 4)[:, 3])]).any(), what
    if a is not None:
        kinds, _ = cr.side_words(sc, pts, ref)
        assert np.array_equal(a[:, 7].view(np.uint32), kinds), what
        o = orc.hit_attributes(np.ascontiguousarray(h))
        f = a.view(np.float32)
        assert np.array_equal(f[:, 0:3].view(np.uint32), o[:, 0:3].view(np.uint32)), what
        assert np.array_equal(f[:, 4:7].view(np.uint32), o[:, 3:6].view(np.uint32)), what
        assert np.array_equal(a[:, 3], o[:, 6].astype(np.int32)), what
        miss = h["inst"] < 0
        assert (a[miss, 0:3] == 0).all() and (a[miss, 4:7] == 0).all() and (a[miss, 7] == 0).all() and (a[miss, 3] == -1).all(), what
    return ref


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_exports_abi_and_null_context():
    assert "rt_closest_point_device" in api.EXPORTS and "rt_closest_point" in api.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^int rt_closest_point_device\(rt_ctx\* ctx, size_t n, const void\* d_points4, uint32_t cull_mask,\s+void\* d_hits, void\* d_attr, "
                     r"void\* hip_stream\);", hdr, re.M)
    assert re.search(r"^int rt_closest_point\(rt_ctx\* ctx, size_t n, const float\* points4_host, uint32_t cull_mask,\s+rt_hit\* out_host, int counting, "
                     r"rt_stats\* stats\);", hdr, re.M)
    L = api.lib()
    assert hasattr(L, "rt_closest_point_device") and hasattr(L, "rt_closest_point") and L.rt_abi_version() == 7
    assert L.rt_closest_point_device(None, 0, None, 0xFF, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_closest_point_device(None, 64, None, 0xFF, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_closest_point(None, 0, None, 0xFF, None, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert hasattr(RtContext, "closest_point_device") and hasattr(RtContext, "closest_point")


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_closest_kernels_keep_the_record_level_budget(target):
    """k_closest_point and its counting form keep the record-level walks' budget (>= 4 waves per SIMD, scratch <= 32 bytes, no spills);
    k_closest_side uses no scratch and spills nothing; one of each in both libraries"""
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    walk = [(n, r) for n, r in kernels.items() if "k_closest_point" in n]
    side = [(n, r) for n, r in kernels.items() if "k_closest_side" in n]
    assert len(walk) == 2 and len(side) == 1, "\n".join(kernels)
    assert sum("k_closest_point_count" in n for n, _ in walk) == 1
    for name, r in walk:
        assert int(r["Occupancy"]) >= 4 and int(r["ScratchSize"]) <= 32 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
    for name, r in side:
        assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)


def teapot_scene(offset=0.0):
    g = host.SceneGeometry([PATHS[0]])
    inst = placed_instances(6, 21, spacing=6.0, n_meshes=1)
    if offset:
        inst["transform"][:, [3, 7, 11]] += np.float32(offset)
    return g.verts, g.idx, g.ranges, inst


@pytest.mark.parametrize("scene_name", ["small", "small+1000", "teapot"])
def test_binary32_restatement_against_binary64(scene_name):
    """t within 1e-5 t + 1e-6 M of the binary64 brute force on every point; the reported triangle touches the binary64 nearest point (is
    the binary64 triangle where one triangle touches it) unless a non-touching runner-up lies within REL; the side equals the binary64
    side wherever |s| > REL |n| |p - v0|; at most 1 % of the points excused by those two clauses together (a point is excused when it
    disagrees and a clause forgives it)"""
    verts, idx, ranges, inst = teapot_scene() if scene_name == "teapot" else small_scene(offset=1000.0 if "+" in scene_name else 0.0)
    sc = cr.Scene(verts, idx, ranges, inst)
    n = 300 if scene_name == "teapot" else 2500
    dets = np.linalg.det(sc.o2w.reshape(-1, 3, 4)[:, :, :3].astype(np.float64))
    for name, pts in point_sets(sc, n, seed=31).items():
        h = cr.brute32(sc, pts)
        r = cr.brute64(sc, pts, picked=(h["inst"], h["prim"]))
        assert (h["inst"] >= 0).all()
        err, tol = np.abs(h["t"].astype(np.float64) - r["t"]), cr.t_tolerance(r["t"], r["mag"])
        print("%s %s: worst t error %.3g of its bound" % (scene_name, name, (err / tol).max()))
        assert (err <= tol).all(), (name, (err / tol).max())
        amb = r["runner"] <= r["t"] * (1 + REL)
        same = r["picked_touches"] & ((r["touching"] != 1) | ((h["inst"] == r["inst"]) & (h["prim"] == r["prim"])))
        assert same[~amb].all(), name
        kinds, _ = cr.side_words(sc, pts, h)
        sure = np.abs(r["side_s"]) > REL * r["side_scale"]
        front64 = ((r["side_s"] * np.sign(dets[h["inst"]])) < 0) != ((sc.flags[h["inst"]] & cr.FLIP) != 0)
        side_same = (kinds == cr.FRONT) == front64
        assert side_same[sure].all(), name
        # a point is excused when it disagrees and a clause forgives it
        excused = (~same | ~side_same).mean()
        print("%s %s: excused %.4f (points a clause could excuse: %.4f)" % (scene_name, name, excused, (amb | ~sure).mean()))
        assert excused <= 0.01, (name, excused)


def test_restatement_misses_radii_and_masks():
    verts, idx, ranges, inst = small_scene()
    sc = cr.Scene(verts, idx, ranges, inst)
    pts = point_sets(sc, 400, seed=41)["volume"]
    full = cr.brute32(sc, pts)
    assert cr.brute32(sc, pts, cand=cr.candidates(sc, pts)).tobytes() == full.tobytes()
    q = pts.copy(); q[:, 3] = full["t"]
    at = cr.brute32(sc, q)     # r_max = t: d2 <= r_max * r_max holds unless the square rounds below d2
    assert (at["inst"] >= 0).mean() > 0.3
    q[:, 3] = np.nextafter(full["t"], INF) * np.float32(1.001)
    assert cr.brute32(sc, q).tobytes() == full.tobytes()
    q[:, 3] = full["t"] * np.float32(0.99)
    m = cr.brute32(sc, q)
    assert (m["inst"] == -1).all() and np.array_equal(m["t"], q[:, 3]) and (m["u"] == 0).all()
    assert (cr.brute32(sc, pts, 0)["inst"] == -1).all()
    one = cr.brute32(sc, pts, 0x01)
    assert ((sc.mask[one["inst"]] & 1) != 0).all() and (one["t"] >= full["t"]).all()
    bad = cr.brute32(sc, invalid_records(pts))
    assert (bad["inst"][:6] == -1).all() and np.array_equal(bad["t"][:6].view(np.uint32), invalid_records(pts)[:6, 3].view(np.uint32))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


def load(c, verts, idx, ranges, inst):
    c.upload_geometry(verts, idx, ranges)
    c.set_instances(inst)
    return cr.Scene(verts, idx, ranges, inst), oracle_scene(verts, idx, ranges, inst)


@pytest.mark.gpu
def test_small_scenes_every_point_set(ctx):
    """near, volume, far, on vertices and edges, inside closed meshes; r_max 0, finite and inf; cull masks 0xFF, single bits, 0; invalid
    records"""
    verts, idx, ranges, inst = small_scene(seed=51)
    sc, orc = load(ctx, verts, idx, ranges, inst)
    sets = point_sets(sc, 3000, seed=52)
    sets["features"] = feature_points(sc, 1000, seed=53)
    octa = np.nonzero(inst["mesh"] == 0)[0]
    rng = np.random.default_rng(54)
    M = np.stack([np.asarray(inst[i]["transform"], np.float64).reshape(3, 4) for i in octa[rng.integers(0, len(octa), 2000)]])
    p = rng.uniform(-0.33, 0.33, (2000, 3))
    sets["inside"] = with_radius(np.einsum("nij,nj->ni", M[:, :, :3], p) + M[:, :, 3], np.inf)
    for name, pts in sets.items():
        ref = check(sc, orc, pts, gpu_closest(ctx, pts), what=name)
        assert (ref["inst"] >= 0).all()
        q = pts.copy()
        k = np.arange(len(q)) % 4
        q[:, 3] = np.where(k == 0, 0.0, np.where(k == 1, ref["t"], np.where(k == 2, ref["t"] * np.float32(0.7), ref["t"] * np.float32(1.5))))
        ref = check(sc, orc, q, gpu_closest(ctx, q), what=name + " radii")
        if name != "features":
            assert (ref["inst"][k == 2] == -1).all() and (ref["inst"][k == 3] >= 0).all()
        for cull in (0x01, 0x02, 0x10, 0x80, 0x5A, 0x00):
            check(sc, orc, pts[:600], gpu_closest(ctx, pts[:600], cull), cull, what="%s cull %#x" % (name, cull))
    bad = invalid_records(sets["volume"])
    ref = check(sc, orc, bad, gpu_closest(ctx, bad), what="invalid records")
    assert (ref["inst"][:6] == -1).all() and (ref["inst"][7:] >= -1).all()
    h, a = gpu_closest(ctx, sets["near"], attributes=False)
    assert a is None and h.tobytes() == cr.brute32(sc, sets["near"]).tobytes()


@pytest.mark.gpu
def test_instance_scale_bound_is_tight(ctx):
    """s_i must be the scale itself for rigid and uniformly scaled instances (a Frobenius-type bound loses sqrt(3), a zero bound all
    pruning).  64 octahedra under rotations times 4, against the same world triangles baked into 64 meshes under identity transforms
    (s_i = 1 for any sound bound): the same surface and nearly the same world boxes, so a tight bound makes the instanced walk cost what
    the baked one costs, up to the shape of the BLAS boxes.  A bound short by sqrt(3) widens every search ball's volume about five
    times; the counts per point are held within a quarter of the baked scene's."""
    verts, idx, ranges = small_meshes(5)
    octa = verts.reshape(-1, 6)[:6]
    inst = placed_instances(64, seed=131, spacing=12.0, n_meshes=1)
    baked_v, baked_i, baked_r = [], [], []
    ident = inst.copy()
    for i in range(len(inst)):
        M = np.asarray(inst[i]["transform"], np.float64).reshape(3, 4)
        U, _, Vt = np.linalg.svd(M[:, :3])
        M[:, :3] = 4.0 * (U @ Vt)
        inst[i]["transform"] = M.astype(np.float32).reshape(12)
        M = np.asarray(inst[i]["transform"], np.float64).reshape(3, 4)
        w = np.concatenate([octa[:, :3].astype(np.float64) @ M[:, :3].T + M[:, 3], octa[:, 3:]], axis=1).astype(np.float32)
        baked_r.append((6 * 6 * i, 24 * i, 8))
        baked_v.append(w); baked_i.append(idx[:24])
        ident[i] = host.make_instance(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), i, i)
    ident["custom_index_and_mask"] = inst["custom_index_and_mask"]
    scenes_ = {"instanced": (verts, idx, ranges[:1], inst),
               "baked": (np.concatenate(baked_v).reshape(-1), np.concatenate(baked_i).astype(np.uint32), baked_r, ident)}
    per_point, pts = {}, None
    for name, (v, ix, rg, records) in scenes_.items():
        sc, orc = load(ctx, v, ix, rg, records)
        if pts is None:
            lo, hi = scene_box(sc)
            pts = with_radius((lo + hi) / 2 + np.random.default_rng(133).uniform(-0.5, 0.5, (20000, 3)) * (hi - lo), np.inf)
        h, st = ctx.closest_point(pts, counting=True)
        assert h[:2000].tobytes() == cr.brute32(sc, pts[:2000]).tobytes(), name
        per_point[name] = (st.node_visits / len(pts), st.tri_tests / len(pts))
        print("%s: %.1f node visits, %.1f triangle tests per point" % ((name,) + per_point[name]))
    for j in range(2):
        assert per_point["instanced"][j] <= 1.25 * per_point["baked"][j], per_point


def degenerate_soup(seed):
    """needles (aspect ~1e-4), zero-area triangles (two equal vertices, three collinear ones, a point) and a few ordinary ones"""
    rng = np.random.default_rng(seed)
    tris = []
    for k in range(48):
        a = rng.uniform(-1, 1, 3)
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        e = np.cross(d, rng.normal(size=3)); e /= np.linalg.norm(e)
        kind = k % 6
        if kind == 0:
            tris.append([a, a + d, a + 0.5 * d + 1e-4 * e])
        elif kind == 1:
            tris.append([a, a + d, a + d])
        elif kind == 2:
            tris.append([a, a + 0.25 * d, a + d])
        elif kind == 3:
            tris.append([a, a, a])
        elif kind == 4:
            tris.append([a, a + 1e-4 * e, a + d])
        else:
            tris.append([a, a + 0.4 * d, a + 0.4 * e])
    pos = np.array(tris, np.float32).reshape(-1, 3)
    verts = np.concatenate([pos, np.tile([[0, 0, 1]], (len(pos), 1))], axis=1).astype(np.float32).reshape(-1)
    return verts, np.arange(len(pos), dtype=np.uint32), [(0, 0, len(tris))]


@pytest.mark.gpu
def test_ties_and_degenerate_triangles(ctx):
    """coincident and mirrored geometry where only (inst, prim) breaks the tie; needles and zero-area triangles: no NaN t, byte-equal"""
    verts, idx, ranges = edge_geometry()
    inst = edge_instances()
    sc, orc = load(ctx, verts, idx, ranges, inst)
    rng = np.random.default_rng(61)
    g = np.linspace(-2.0, 2.0, 9)
    grid = np.array([[x, y, z] for x in g for y in g for z in (0.0, 0.5, -0.25)])
    pts = with_radius(np.concatenate([grid, rng.uniform(-2.5, 2.5, (1500, 3)) * [1, 1, 0.3]]), np.inf)
    ties = 0
    for cull in (0xFF, 0x01, 0x02, 0x03, 0x06, 0x1C, 0x20, 0x3E):
        ref = check(sc, orc, pts, gpu_closest(ctx, pts, cull), cull, what="ties cull %#x" % cull)
        adm = sc.admitted(cull)
        # a tie: another admitted triangle at the same binary32 d2
        d2, _, _ = cr.tri_d2(tuple(pts[:200, k][:, None] for k in range(3)), tuple(sc.a[adm, k][None] for k in range(3)),
                             tuple(sc.ab[adm, k][None] for k in range(3)), tuple(sc.ac[adm, k][None] for k in range(3)))
        ties += ((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum()
    assert ties > 500, ties
    verts, idx, ranges = degenerate_soup(62)
    inst = placed_instances(12, 63, spacing=2.5, n_meshes=1)
    sc, orc = load(ctx, verts, idx, ranges, inst)
    sets = point_sets(sc, 2500, seed=64)
    sets["features"] = feature_points(sc, 800, seed=65)
    for name, pts in sets.items():
        h, a = gpu_closest(ctx, pts, attributes=False)
        assert not np.isnan(h["t"]).any()
        check(sc, orc, pts, (h, None), what="degenerate " + name)


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "1", "2", "3"])
def test_tree_independence(builder, monkeypatch):
    """the same points over every BLAS builder, host and device instance records with their refits, and a refitted BLAS: one brute force"""
    import torch
    from tests.test_blas_refit import deform, with_mesh
    verts, idx, ranges, inst = small_scene(seed=71)
    geom = types.SimpleNamespace(verts=verts, idx=idx, ranges=ranges)
    rng = np.random.default_rng(72)
    moved = inst.copy()
    moved["transform"][:, [3, 7, 11]] += rng.uniform(-0.3, 0.3, (len(inst), 3)).astype(np.float32)
    sc0 = cr.Scene(verts, idx, ranges, inst)
    pts = np.concatenate(list(point_sets(sc0, 1200, seed=73).values()) + [feature_points(sc0, 300, seed=74)])
    c = RtContext(0)
    try:
        use_builder(c, builder, monkeypatch)
        c.upload_geometry(verts, idx, ranges)
        for source in ("host", "device"):
            for records, update in ((inst, False), (moved, True)):
                if source == "host":
                    c.set_instances(records, update=update)
                else:
                    torch.cuda.synchronize()
                    c.set_instances_device(dev_inst(records), update=update)
                sc, orc = cr.Scene(verts, idx, ranges, records), oracle_scene(verts, idx, ranges, records)
                for cull in (0xFF, 0x5A):
                    check(sc, orc, pts, gpu_closest(c, pts, cull), cull, "%s records, update %d, builder %s" % (source, update, builder))
        t = deform(geom, 0, amp=0.2)
        torch.cuda.synchronize()
        c.refit_blas_device(0, t)
        torch.cuda.synchronize()
        c.set_instances_device(dev_inst(inst))
        v2 = with_mesh(geom, verts, 0, t)
        check(cr.Scene(v2, idx, ranges, inst), oracle_scene(v2, idx, ranges, inst), pts, gpu_closest(c, pts), what="refit, builder %s" % builder)
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [1000.0, 10000.0])
def test_translated_scene_and_far_points(ctx, offset):
    """the scene 1000 and 10000 units from the origin, and points 1e4 away from it: the box bound's slack must cover the binary32 d2"""
    verts, idx, ranges, inst = small_scene(seed=81, offset=offset)
    sc, orc = load(ctx, verts, idx, ranges, inst)
    sets = point_sets(sc, 2500, seed=82)
    rng = np.random.default_rng(83)
    d = rng.normal(size=(2500, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    lo, hi = scene_box(sc)
    sets["1e4 away"] = with_radius((lo + hi) / 2 + d * 1e4, np.inf)
    sets["features"] = feature_points(sc, 600, seed=84)
    for name, pts in sets.items():
        ref = check(sc, orc, pts, gpu_closest(ctx, pts), what="offset %g %s" % (offset, name))
        q = pts.copy(); q[:, 3] = ref["t"] * np.float32(1.25)
        check(sc, orc, q, gpu_closest(ctx, q), what="offset %g %s radii" % (offset, name))


def cfg3_point_sets(sc, n, seed):
    """the cost table's sets: (a) surface samples displaced by up to 1 % of the diagonal, (b) uniform in twice the scene box, (c) set (b)
    with r_max = 1 % of the diagonal"""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(sc)
    c, diag = (lo + hi) / 2, np.linalg.norm(hi - lo)
    b = c + rng.uniform(-1, 1, (n, 3)) * (hi - lo)
    return {"a": with_radius(surface_points(sc, n, rng, 0.01 * diag), np.inf), "b": with_radius(b, np.inf), "c": with_radius(b, 0.01 * diag)}


@pytest.fixture(scope="module")
def cfg3():
    wl = workloads.make("cfg3", os.path.join(ROOT, "resources"), mesh="standin")
    g = wl.geometry
    return wl, cr.Scene(g.verts, g.idx, g.ranges, wl.instances), oracle_scene(g.verts, g.idx, g.ranges, wl.instances)


@pytest.mark.gpu
def test_cfg3_scene(ctx, cfg3):
    """2048 points of each cost-table set against the brute force; a 1 M-point call whose every record satisfies the invariants
    (t <= r_max; t equals the binary64 distance from the point to the (u, v) point of the reported triangle within 1e-5 t + 1e-6 M; the
    sampled indices byte-equal); the host form's counting: the tree prunes (mean triangle tests per point < triangles / 100)"""
    wl, sc, orc = cfg3
    wl.apply(ctx)
    assert sc.n_tris == sum(wl.geometry.ranges[int(r["mesh"])][2] for r in wl.instances) > 300_000
    for name, pts in cfg3_point_sets(sc, 2048, seed=91).items():
        ref = check(sc, orc, pts, gpu_closest(ctx, pts), what="cfg3 set " + name, cand=cr.candidates(sc, pts))
        assert (ref["inst"] >= 0).mean() > (0.9 if name != "c" else 0.0)
    n = 1 << 20
    sets = cfg3_point_sets(sc, n // 4, seed=92)
    pts = np.concatenate([sets["a"], sets["a"][::-1], sets["b"], sets["c"]])
    h, _ = gpu_closest(ctx, pts, attributes=False)
    hit = h["inst"] >= 0
    assert hit[: n // 2].all() and (h["t"] <= pts[:, 3]).all() and (h["t"][~hit] == pts[~hit, 3]).all()
    first = np.concatenate([[0], np.cumsum(np.bincount(sc.inst, minlength=len(sc.mask)))])
    k = first[h["inst"][hit]] + h["prim"][hit]
    u, v = h["u"][hit].astype(np.float64)[:, None], h["v"][hit].astype(np.float64)[:, None]
    q = sc.A[k] + u * (sc.B[k] - sc.A[k]) + v * (sc.C[k] - sc.A[k])
    p = pts[hit, :3].astype(np.float64)
    d = np.linalg.norm(p - q, axis=1)
    mag = np.maximum(np.abs(p).max(-1), np.maximum(np.maximum(np.abs(sc.A[k]).max(-1), np.abs(sc.B[k]).max(-1)), np.abs(sc.C[k]).max(-1)))
    assert (np.abs(h["t"][hit] - d) <= cr.t_tolerance(d, mag)).all()
    assert (u >= 0).all() and (v >= 0).all() and (u + v <= 1 + 1e-6).all()
    sample = np.random.default_rng(93).choice(n, 2048, replace=False)
    assert h[sample].tobytes() == cr.brute32(sc, pts[sample], cand=cr.candidates(sc, pts[sample])).tobytes()
    hh, st = ctx.closest_point(sets["a"][:200_000], counting=True)
    assert hh.tobytes() == h[:200_000].tobytes()
    per_point = st.tri_tests / 200_000
    print("cfg3 set (a): %.1f triangle tests, %.1f node visits per point" % (per_point, st.node_visits / 200_000))
    assert 0 < per_point < sc.n_tris / 100 and st.node_visits > 0


@pytest.mark.gpu
def test_plumbing(ctx):
    """host form = device form; out= reuse; stream order behind a slow queue on a side stream; interleaving with rt_intersect_device and
    rt_shade_rays_device; n == 0"""
    import torch
    from tests.test_ray_query import mixed_rays
    sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
    g = sp.geom
    sc, orc = load(ctx, g.verts, g.idx, g.ranges, sp.instances)
    ctx.set_uniforms(sp.uniforms)
    pts = np.concatenate(list(point_sets(sc, 700, seed=101).values()))
    cand = cr.candidates(sc, pts)
    ref = check(sc, orc, pts, gpu_closest(ctx, pts), what="two objects", cand=cand)
    hh, st = ctx.closest_point(pts)
    assert hh.tobytes() == ref.tobytes() and st.node_visits == 0
    hc, st = ctx.closest_point(pts, counting=True)
    assert hc.tobytes() == ref.tobytes() and st.node_visits > 0 and st.tri_tests > 0
    assert ctx.closest_point(pts, cull_mask=0)[0]["inst"].max() == -1
    # out= reuse
    src = dev(pts)
    hits = torch.empty((len(pts), 5), dtype=torch.int32, device="cuda:0"); attr = torch.empty((len(pts), 8), dtype=torch.int32, device="cuda:0")
    res = ctx.closest_point_device(src, attributes=True, out=(hits, attr))
    assert res.hits.data_ptr() == hits.data_ptr() and res.attr.data_ptr() == attr.data_ptr()
    assert res.numpy()[0].tobytes() == ref.tobytes()
    with pytest.raises(ValueError):
        ctx.closest_point_device(src, out=(hits[:-1], None))
    # stream order
    rays = torch.from_numpy(mixed_rays(len(pts), seed=102)).to("cuda:0")
    closest = ctx.intersect_device(rays).numpy()[0]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = slow_queue(torch, 12)
        p = (src + (a[0, 0] != a[0, 0]).to(torch.float32) * 0).contiguous()   # made behind the queue, on s
        r1 = ctx.closest_point_device(p, attributes=True, stream=s)
        q1 = ctx.intersect_device(rays, stream=s)
        img = ctx.shade_rays_device(rays, stream=s) if hasattr(ctx, "shade_rays_device") else None
        r2 = ctx.closest_point_device(p, stream=s)
        p.zero_()                                                             # overwritten right after the calls
        h1, h2, hq = r1.hits.clone(), r2.hits.clone(), q1.hits.clone()
    s.synchronize()
    assert img is not None
    for hcopy in (h1, h2):
        assert hcopy.cpu().numpy().view(HIT_DTYPE).reshape(-1).tobytes() == ref.tobytes()
    assert hq.cpu().numpy().view(HIT_DTYPE).reshape(-1).tobytes() == closest.tobytes()
    # n == 0
    e = ctx.closest_point_device(torch.empty((0, 4), dtype=torch.float32, device="cuda:0"), attributes=True)
    assert e.hits.shape == (0, 5) and e.attr.shape == (0, 8)
    assert len(ctx.closest_point(np.zeros((0, 4), np.float32))[0]) == 0


@pytest.mark.gpu
def test_frame_in_flight_beside_a_closest_point_query():
    """a frame in flight on the context's slot is neither waited for nor changed: its pixels equal the frame rendered alone"""
    import torch
    from tests.test_ray_query import W, H, two_objects
    base = RtContext(0)
    slot = base.frame_slot()
    try:
        sp = two_objects(base)
        slot.set_instances(sp.instances)
        slot.set_uniforms(sp.uniforms)
        before = base.trace(W, H)[0]
        sc, orc = cr.Scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances), oracle_scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances)
        pts = point_sets(sc, 1500, seed=111)["near"]
        src = dev(pts)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        slot.trace_async(W, H)
        with torch.cuda.stream(s):
            slow_queue(torch, 4)
            res = base.closest_point_device(src, attributes=True, stream=s)
        during, _ = slot.trace_wait()
        after = base.trace(W, H)[0]
        s.synchronize()
        assert np.array_equal(during.view(np.uint32), before.view(np.uint32))
        assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
        check(sc, orc, pts, res.numpy(), what="beside frames", cand=cr.candidates(sc, pts))
    finally:
        slot.close()
        base.close()


def _raw(c, n, pts, cull, hits, attr):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_closest_point_device(c.h, n, p(pts), cull, p(hits), p(attr), None)


@pytest.mark.gpu
def test_error_statuses():
    import torch
    from tests.test_blas_refit import span
    sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
    sc = cr.Scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances)
    pts_np = point_sets(sc, 500, seed=121)["near"]
    ref = cr.brute32(sc, pts_np, cand=cr.candidates(sc, pts_np))
    pts = dev(pts_np)
    n = pts.shape[0]
    hits = torch.empty((n + 1, 5), dtype=torch.int32, device="cuda:0")
    attr = torch.empty((n + 1, 8), dtype=torch.int32, device="cuda:0")
    P_, H_, A_ = pts.data_ptr(), hits.data_ptr(), attr.data_ptr()
    c = RtContext(0)

    def err(args, code, text):
        assert _raw(c, *args) == code, args
        msg = c.L.rt_last_error(c.h).decode()
        assert text in msg, (args, msg)

    def ok():
        assert c.closest_point_device(pts).numpy()[0].tobytes() == ref.tobytes()

    try:
        err((n, P_, 0xFF, H_, 0), RT_ERR_NOT_READY, "")   # no geometry
        c.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        err((n, P_, 0xFF, H_, 0), RT_ERR_NOT_READY, "")   # no TLAS
        c.set_instances(sp.instances)
        c.set_uniforms(sp.uniforms)
        ok()
        bad = [((0xFFFFFF00, P_, 0xFF, H_, 0), "too many points"), ((n, P_, 0x100, H_, 0), "cull_mask"), ((n, 0, 0xFF, H_, 0), "null point/hit pointers"),
               ((n, P_, 0xFF, 0, 0), "null point/hit pointers"), ((n, P_ + 4, 0xFF, H_, 0), "aligned"), ((n, P_, 0xFF, H_ + 2, 0), "aligned"),
               ((n, P_, 0xFF, H_, A_ + 4), "aligned")]
        host_buf = np.zeros((n + 1, 8), np.float32)
        pinned = torch.zeros((n, 8), dtype=torch.float32).pin_memory()
        for ptr in ((host_buf.ctypes.data + 15) & ~15, pinned.data_ptr()):   # (16-byte aligned: only the memory kind is wrong)
            bad += [((n, ptr, 0xFF, H_, 0), "device memory of the context's GPU"), ((n, P_, 0xFF, ptr, 0), "device memory of the context's GPU"),
                    ((n, P_, 0xFF, H_, ptr), "device memory of the context's GPU")]
        for args, text in bad:
            err(args, RT_ERR_INVALID_ARGUMENT, text)
            ok()
        out = np.zeros(n, HIT_DTYPE)
        assert c.L.rt_closest_point(c.h, n, None, 0xFF, out.ctypes.data_as(ctypes.c_void_p), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_closest_point(c.h, n, pts_np.ctypes.data_as(ctypes.c_void_p), 0x100, out.ctypes.data_as(ctypes.c_void_p), 0, None) == RT_ERR_INVALID_ARGUMENT
        ok()
        assert _raw(c, 0, 0, 0xFF, 0, 0) == 0   # n == 0 enqueues nothing and needs no pointers
        with pytest.raises(ValueError):
            c.closest_point_device(pts.cpu())
        with pytest.raises(ValueError):
            c.closest_point_device(torch.zeros((4, 8), dtype=torch.float32, device="cuda:0"))
        with pytest.raises(RtError) as e:
            c.closest_point_device(pts, cull_mask=0x1FF)
        assert e.value.code == RT_ERR_INVALID_ARGUMENT
        ok()
        # not ready: a stale TLAS after a BLAS refit, then a frame batch
        ff, nf = span(sp.geom, 1)
        v = torch.from_numpy(sp.geom.verts[ff:ff + nf].copy()).to("cuda:0")
        torch.cuda.synchronize()
        c.refit_blas_device(1, v)
        err((n, P_, 0xFF, H_, 0), RT_ERR_NOT_READY, "")
        c.set_instances(sp.instances)
        ok()
        c.set_batch(np.stack([sp.instances, sp.instances]), np.stack([sp.uniforms, sp.uniforms]).reshape(-1))
        err((n, P_, 0xFF, H_, 0), RT_ERR_NOT_READY, "")
        c.set_instances(sp.instances)
        ok()
    finally:
        c.close()
    # trace_variant != 0 (alt library only: the product refuses the parameter itself)
    a = RtContext(0, variant="alt")
    try:
        a.set_param("blas_builder", 0)
        a.set_param("trace_variant", 1)
        a.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        a.set_instances(sp.instances)
        c = a
        err((n, P_, 0xFF, H_, 0), RT_ERR_INVALID_ARGUMENT, "trace_variant 0")
        a.set_param("trace_variant", 0)
        a.set_instances(sp.instances)
        ok()
    finally:
        a.close()
