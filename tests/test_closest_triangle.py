"""rt_closest_triangle_device / rt_closest_triangle: the nearest pair of every query triangle and the scene's surface.

tests/triangle_distance_reference.py holds the three references: brute32, the canonical binary32 feature sequence and key of
include/rt_api.h and DESIGN.md §5 "Closest points of triangles" restated in numpy over every triangle; brute64, the minimum over the six
edge-against-triangle pairs of a binary64 ternary search; altproj64, alternating binary64 projections.  The CPU part holds brute32 to
brute64 (and brute64 to altproj64); the GPU part holds the library to brute32 byte for byte: hits, parameters, attributes (against the
oracle's hit_attributes of the returned records) and side words, under every tree the library can build, far from the origin, on
degenerate geometry, in the spill half of the stack, against the point, segment and overlap queries, and the plumbing of a device query.

Identity against binary64 is test_closest_segment.py's rule (the reported triangle touches the scene's point of the binary64 nearest
pair and is the binary64 triangle where only one touches it; at most 1 % of the records excused by a runner-up within REL) for the
records whose binary64 distance exceeds the tolerance.  A record whose binary64 distance is zero within the tolerance cuts or touches
the surface, often several triangles of it: there the contract lets the key decide among residues, so the test asks instead that the
reported triangle's own binary64 distance to the query be within the bound."""
import ctypes
import itertools
import os
import re
import types

import numpy as np
import pytest

from tests import closest_reference as cr
from tests import scenes
from tests import segment_reference as sgr
from tests import triangle_distance_reference as tdr
from tests.query_reference import REL
from tests.test_closest_point import degenerate_soup, scene_box, small_scene, surface_points, teapot_scene
from tests.test_closest_segment import inside_points, unit
from tests.test_ray_query import PATHS, dev_inst, slow_queue
from tests.test_ray_query_oracle import oracle_scene, placed_instances, use_builder
from vulkan_raytracing_amd import RtContext, api
from vulkan_raytracing_amd.api import HIT_DTYPE, RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
INF = np.float32(np.inf)
F = np.float32
# |t32 - t64| <= K (1e-5 t + 1e-6 M): the smallest power of two that holds on every committed set is K_MEASURED (the comparison tests
# print the worst ratio of every set; DESIGN.md §5 has the table); the bound asserted is four times it, the margin the segment query
# took.  The eight sets of 400 stay below 0.12; the worst committed record, 1.17, is in WORST_SET: a query face 10 units across cut by
# a scene edge, whose crossing is measured against that face by closest_tri to a few binary32 spacings of the FACE's extent, which may
# be twice M.  Touching pairs whose planes are within SHALLOW radians are held to K 2^-12 M.
K_MEASURED = 2.0
K = 4.0 * K_MEASURED
WORST_SET = dict(scene_seed=91, set_seed=92, n=250, name="across")
SHALLOW = 2.0 ** -8


# ---- scenes and record sets ---------------------------------------------------------------------------------------------------

def records(p0, p1, p2, r=np.inf):
    p0 = np.asarray(p0, np.float64).reshape(-1, 3)
    out = np.zeros((len(p0), 12), F)
    out[:, 0:3] = p0; out[:, 4:7] = np.asarray(p1, np.float64).reshape(-1, 3); out[:, 8:11] = np.asarray(p2, np.float64).reshape(-1, 3)
    out[:, 3] = r
    return out


def triangle_sets(sc, n, seed, closed):
    """small triangles near the surface; triangles across the scene (many cut it); triangles inside closed meshes; triangles parallel to a
    face; coplanar with a face, outside it and overlapping it; with an edge parallel to a scene edge; a small scene triangle poking
    through a large query face, and a small query poking through a scene face; needle queries.  r_max = inf"""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(sc)
    c, diag = (lo + hi) / 2, np.linalg.norm(hi - lo)
    sets = {}
    p = surface_points(sc, n, rng, 0.02 * diag)
    sets["near"] = records(p, p + unit(rng, n) * rng.uniform(0.001, 0.03, (n, 1)) * diag, p + unit(rng, n) * rng.uniform(0.001, 0.03, (n, 1)) * diag)
    sets["across"] = records(*(c + rng.uniform(-0.55, 0.55, (n, 3)) * (hi - lo) for _ in range(3)))
    p = inside_points(sc, n, rng, closed)
    sets["inside"] = records(p, p + unit(rng, n) * rng.uniform(0.005, 0.05, (n, 1)), p + unit(rng, n) * rng.uniform(0.005, 0.05, (n, 1)))
    k = rng.integers(0, sc.n_tris, n)
    A, B, C = sc.A[k], sc.B[k], sc.C[k]
    N = np.cross(B - A, C - A)
    with np.errstate(invalid="ignore"):      # (a zero-area scene triangle gives NaN records: invalid ones, answered by the miss form)
        N /= np.linalg.norm(N, axis=1, keepdims=True)

    def bary(u, v):
        return A + u * (B - A) + v * (C - A)
    uv = rng.uniform(-0.5, 1.5, (3, 2, n, 1))
    h = N * rng.uniform(0.001, 0.05, (n, 1)) * diag * np.where(rng.uniform(size=(n, 1)) < 0.5, -1.0, 1.0)
    sets["parallel"] = records(*(bary(uv[j, 0], uv[j, 1]) + h for j in range(3)))
    # coplanar: even records outside (all three beyond the edge BC), odd ones with P0 inside the face
    outside = (np.arange(n) % 2 == 0)[:, None]
    uv = np.where(outside, rng.uniform(0.7, 2.0, (3, 2, n, 1)), rng.uniform(-1.0, 2.0, (3, 2, n, 1)))
    uv[0] = np.where(outside, uv[0], rng.uniform(0.1, 0.4, (2, n, 1)))
    sets["coplanar"] = records(*(bary(uv[j, 0], uv[j, 1]) for j in range(3)))
    e0 = np.where((k % 3 == 0)[:, None], A, np.where((k % 3 == 1)[:, None], B, C))
    e1 = np.where((k % 3 == 0)[:, None], B, np.where((k % 3 == 1)[:, None], C, A))
    off = unit(rng, n) * rng.uniform(0.0, 0.01, (n, 1)) * diag
    a, b = rng.uniform(-0.3, 0.6, (n, 1)), rng.uniform(0.4, 1.3, (n, 1))
    q0 = e0 + a * (e1 - e0) + off
    sets["edge-parallel"] = records(q0, e0 + b * (e1 - e0) + off, q0 + off * 3 + unit(rng, n) * rng.uniform(0.01, 0.1, (n, 1)) * diag)
    # poke: even records a large query face through the centroid of a scene triangle, in a random orientation (the scene triangle's edges
    # cross the query's plane, the query's edges pass far outside); odd ones a small query through an interior point of the scene triangle
    cen = (A + B + C) / 3
    size = np.maximum(np.linalg.norm(B - A, axis=1), np.linalg.norm(C - A, axis=1))[:, None]
    d0 = unit(rng, n)
    d1 = np.cross(d0, unit(rng, n)); d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    big = (np.arange(n) % 2 == 0)[:, None]
    R = np.where(big, rng.uniform(4.0, 8.0, (n, 1)), rng.uniform(0.02, 0.1, (n, 1))) * size
    at = np.where(big, cen, bary(rng.uniform(0.25, 0.4, (n, 1)), rng.uniform(0.25, 0.4, (n, 1)))) + (d0 + d1) * R * rng.uniform(-0.1, 0.1, (n, 1))
    sets["poke"] = records(at + R * d0, at + R * (-0.5 * d0 + 0.87 * d1), at + R * (-0.5 * d0 - 0.87 * d1))
    p = surface_points(sc, n, rng, 0.03 * diag)
    d = unit(rng, n) * rng.uniform(0.01, 0.2, (n, 1)) * diag
    # (a needle 1e-5 of its length wide, but no thinner than 16 binary32 spacings of its coordinates: it has to survive the rounding of
    # the record to binary32 as a needle, not as three collinear points plus noise)
    width = np.maximum(1e-5 * np.linalg.norm(d, axis=1, keepdims=True), 2.0 ** -19 * np.abs(p).max(axis=1, keepdims=True))
    sets["needles"] = records(p, p + d, p + rng.uniform(0.1, 0.9, (n, 1)) * d + unit(rng, n) * width)
    return sets


FLAT_SETS = ("parallel", "coplanar", "edge-parallel")     # the nearest pair is a continuum by construction
# No set is excluded from the binary64 comparison of t: the needle queries stay within the bound (the needle SOUP is a scene of the GPU
# tests only, as it is for the other queries: binary64 has no meaningful nearest triangle among zero-area ones).  One set is excluded
# from the identity assertion (its share of disagreeing records is still held to the 1 % cap), and stays in every other check and, at the
# origin and 1000 and 10 000 units out, in the byte-for-byte GPU tests:
IDENTITY_EXCLUDED = {
    ("small+1000", "needles"):
        "record 85: its two nearest triangles (instance 4, primitives 6 and 2) are 0.09378116 and 0.09379105 away in binary64, 9.89e-6 apart "
        "where REL t is 9.38e-6, so the runner-up is just out of reach; but 1000 units out one binary32 spacing of the coordinates is "
        "1.2e-4, the contract's triangle is the binary32 (a, ab, ac) and brute64's the binary64 image of the packet, up to half a spacing "
        "apart per coordinate, so the two cannot be told apart there and the restatement reports primitive 2",
}
# Pairs of test_binary64_decomposition_against_alternating_projections on which the projections do not reach the tolerance in 2000 rounds:
# the two triangles touch (binary64 distance 3e-15) and the projections converge sublinearly: measured beyond brute64 by 217 and 399
# tolerances after 2000 rounds, 2.8 and 133 after 20 000, within it and at 1.0 after 100 000.
SLOW_PAIRS = {"near": (256,), "poke": (240,)}


def feature_triangles(sc, n, seed):
    """a vertex exactly on a world vertex, a vertex (to binary32 rounding) on an edge, an edge from vertex to vertex, and degenerate
    queries: two equal vertices, three collinear ones"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, sc.n_tris, n)
    on_v = np.where((k % 3 == 0)[:, None], sc.A[k], np.where((k % 3 == 1)[:, None], sc.B[k], sc.C[k]))
    on_e = sc.A[k] + rng.uniform(size=(n, 1)) * (sc.B[k] - sc.A[k])
    far, far2 = on_v + unit(rng, n) * rng.uniform(0.05, 1.0, (n, 1)), on_v + unit(rng, n) * rng.uniform(0.05, 1.0, (n, 1))
    k2 = rng.integers(0, sc.n_tris, n)
    two = records(far, far, far2)
    two[1::3, 8:11], two[1::3, 4:7] = two[1::3, 4:7].copy(), two[1::3, 8:11].copy()      # P0 == P2 (the others P0 == P1)
    two[2::3, 0:3] = two[2::3, 8:11]; two[2::3, 8:11] = two[2::3, 4:7]                    # P1 == P2
    f32 = lambda x: np.asarray(x, F).astype(np.float64)   # noqa: E731
    line = records(far, f32(far) + (f32(far2) - f32(far)) * 0.5, far2)
    return np.concatenate([records(on_v, far, far2), records(far, on_e, far2), records(on_v, sc.C[k2], far), two, line])


def invalid_records(s):
    """records the contract answers with the miss form: NaN / inf in each vertex, r_max of -1, NaN and -inf; then valid ones"""
    q = np.array(s[:16], F).copy()
    q[0, 0] = np.nan; q[1, 1] = np.inf; q[2, 2] = -np.inf; q[3, 4] = np.nan; q[4, 5] = -np.inf; q[5, 6] = np.inf
    q[6, 8] = np.nan; q[7, 9] = np.inf; q[8, 10] = -np.inf
    q[9, 3] = -1.0; q[10, 3] = np.nan; q[11, 3] = -np.inf
    q[12, 3] = F(-0.0); q[13, 3] = 3e38; q[14, 7] = np.nan; q[15, 11] = np.inf   # (words 7 and 11 are ignored)
    return q


N_INVALID = 12


def dev(s):
    import torch
    return torch.from_numpy(np.ascontiguousarray(s, F).reshape(-1, 12)).to("cuda:0")


def gpu_triangles(ctx, tris, cull=0xFF, attributes=True, params=True):
    import torch
    res = ctx.closest_triangle_device(dev(tris), cull_mask=cull, attributes=attributes, params=params)
    torch.cuda.synchronize()
    h, a = res.numpy()
    return h, a, (res.quv.cpu().numpy() if res.quv is not None else None)


def check(sc, orc, tris, got, cull=0xFF, what=""):
    """the GPU's (hits, attributes, (qu, qv)) against brute32 byte for byte; attributes against orc.hit_attributes of the returned records
    and the restated side words"""
    h, a, quv = got
    ref, q_ref, _ = tdr.brute32(sc, tris, cull)
    if h.tobytes() != ref.tobytes():
        bad = np.nonzero((h.view(np.uint8).reshape(len(h), -1) != ref.view(np.uint8).reshape(len(h), -1)).any(axis=1))[0]
        raise AssertionError("%s: %d records differ from the brute force, first %d: triangle %s gpu %s reference %s" %
                             (what, len(bad), bad[0], np.asarray(tris).reshape(-1, 12)[bad[0]], h[bad[0]], ref[bad[0]]))
    if quv is not None:
        assert quv.tobytes() == q_ref.tobytes(), (what, np.nonzero((quv.view(np.uint32) != q_ref.view(np.uint32)).any(axis=1))[0][:5])
        assert not np.signbit(quv).any() and (quv >= 0).all() and (quv <= 1).all(), what
    r_max = np.asarray(tris, F).reshape(-1, 12)[:, 3]
    assert not np.isnan(h["t"][~np.isnan(r_max)]).any(), what
    if a is not None:
        kinds, _ = tdr.side_words(sc, tris, ref, q_ref)
        assert np.array_equal(a[:, 7].view(np.uint32), kinds), what
        o = orc.hit_attributes(np.ascontiguousarray(h))
        f = a.view(F)
        assert np.array_equal(f[:, 0:3].view(np.uint32), o[:, 0:3].view(np.uint32)), what
        assert np.array_equal(f[:, 4:7].view(np.uint32), o[:, 3:6].view(np.uint32)), what
        assert np.array_equal(a[:, 3], o[:, 6].astype(np.int32)), what
        miss = h["inst"] < 0
        assert (a[miss, 0:3] == 0).all() and (a[miss, 4:7] == 0).all() and (a[miss, 7] == 0).all() and (a[miss, 3] == -1).all(), what
    return ref, q_ref


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_exports_abi_null_context_and_record_packing():
    assert "rt_closest_triangle_device" in api.EXPORTS and "rt_closest_triangle" in api.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^int rt_closest_triangle_device\(rt_ctx\* ctx, size_t n, const void\* d_tris12, uint32_t cull_mask,\s+void\* d_hits, void\* d_attr, "
                     r"void\* d_params, void\* hip_stream\);", hdr, re.M)
    assert re.search(r"^int rt_closest_triangle\(rt_ctx\* ctx, size_t n, const float\* tris12_host, uint32_t cull_mask,\s+rt_hit\* out_host, "
                     r"float\* params_host, int counting, rt_stats\* stats\);", hdr, re.M)
    L = api.lib()
    assert hasattr(L, "rt_closest_triangle_device") and hasattr(L, "rt_closest_triangle") and L.rt_abi_version() == 7
    assert L.rt_closest_triangle_device(None, 0, None, 0xFF, None, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_closest_triangle_device(None, 64, None, 0xFF, None, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_closest_triangle(None, 0, None, 0xFF, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert hasattr(RtContext, "closest_triangle_device") and hasattr(RtContext, "closest_triangle")
    v = np.arange(12, dtype=F).reshape(4, 3)
    f = np.array([[0, 1, 2], [3, 2, 1]])
    today = np.zeros((2, 3, 4), F); today[:, :, :3] = v[f]         # what triangle_records(vertices, faces) has always written
    assert api.triangle_records(v, f).tobytes() == today.reshape(2, 12).tobytes()
    rec = api.triangle_records(v, f, r_max=2.5)
    assert rec.dtype == F and rec[:, 3].tolist() == [2.5, 2.5] and (rec[:, [7, 11]] == 0).all() and np.array_equal(np.delete(rec, 3, 1), np.delete(today.reshape(2, 12), 3, 1))
    assert api.triangle_records(v, f, r_max=np.array([1.0, np.inf]))[:, 3].tolist() == [1.0, np.inf]
    import torch
    rt = api.triangle_records(torch.from_numpy(v), torch.from_numpy(f), r_max=torch.tensor([1.0, 3.0]))
    assert isinstance(rt, torch.Tensor) and rt[:, 3].tolist() == [1.0, 3.0] and np.array_equal(np.delete(rt.numpy(), 3, 1), np.delete(today.reshape(2, 12), 3, 1))
    assert api.triangle_records(torch.from_numpy(v), torch.from_numpy(f)).numpy().tobytes() == today.reshape(2, 12).tobytes()


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_triangle_kernels_keep_the_record_level_budget(target):
    """k_closest_triangle and its counting form keep the record-level walks' budget (>= 4 waves per SIMD, scratch <= 32 bytes, no
    spills); k_triangle_side uses no scratch and spills nothing; one of each in both libraries"""
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    walk = [(n, r) for n, r in kernels.items() if "k_closest_triangle" in n]
    side = [(n, r) for n, r in kernels.items() if "k_triangle_side" in n]
    assert len(walk) == 2 and len(side) == 1, "\n".join(kernels)
    assert sum("k_closest_triangle_count" in n for n, _ in walk) == 1
    for name, r in walk:
        assert int(r["Occupancy"]) >= 4 and int(r["ScratchSize"]) <= 32 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
    for name, r in side:
        assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)


def closed_of(inst):
    return np.nonzero(inst["mesh"] == 0)[0]


def cpu_scene(scene_name):
    verts, idx, ranges, inst = teapot_scene() if scene_name == "teapot" else small_scene(offset=1000.0 if "+" in scene_name else 0.0)
    sc = cr.Scene(verts, idx, ranges, inst)
    closed = np.arange(len(inst)) if scene_name == "teapot" else np.nonzero(inst["mesh"] == 0)[0]
    return sc, closed


def plane_sines(sc, tris, tri):
    """the sine of the angle between the query's plane and the plane of scene triangle `tri` (NaN for a zero-area one of either)"""
    P0, P1, P2 = tdr.vertices64(tris)
    tri = np.clip(tri, 0, sc.n_tris - 1)
    Nq, Nt = np.cross(P1 - P0, P2 - P0), np.cross(sc.B[tri] - sc.A[tri], sc.C[tri] - sc.A[tri])
    with np.errstate(all="ignore"):
        return np.linalg.norm(np.cross(Nq, Nt), axis=1) / (np.linalg.norm(Nq, axis=1) * np.linalg.norm(Nt, axis=1))


def shallow_touches(sc, tris, r, picked):
    """(n,) bool: the query's plane lies within SHALLOW radians of the plane of a triangle it touches (its binary64 distance to that
    triangle is within the plain tolerance): the binary64 nearest triangle or the reported one"""
    first = np.concatenate([[0], np.cumsum(np.bincount(sc.inst, minlength=len(sc.mask)))])
    tol = cr.t_tolerance(r["t"], r["mag"])
    out = np.zeros(len(tol), bool)
    for tri, dist in ((r["tri"], r["t"]), (first[np.clip(picked["inst"], 0, None)] + picked["prim"], r["picked_t"])):
        out |= (dist <= tol) & ~(plane_sines(sc, tris, tri) >= SHALLOW)
    return out


_CPU = {}


def cpu_results(scene_name):
    """{set: (triangles, brute32 hits, brute32 (qu, qv), brute64 dict)} of a CPU scene, computed once"""
    if scene_name not in _CPU:
        sc, closed = cpu_scene(scene_name)
        out = {}
        for name, tris in triangle_sets(sc, 60 if scene_name == "teapot" else 400, seed=331, closed=closed).items():
            h, quv, _ = tdr.brute32(sc, tris)
            out[name] = (tris, h, quv, tdr.brute64(sc, tris, picked=(h["inst"], h["prim"])))
        _CPU[scene_name] = (sc, out)
    return _CPU[scene_name]


def t_bound(r, shallow):
    """the bound on |t32 - t64|: K (1e-5 t + 1e-6 M), for shallow touches K 2^-12 M"""
    return np.where(shallow, K * 2.0 ** -12 * r["mag"], K * cr.t_tolerance(r["t"], r["mag"]))


def identity(set_name, h, r):
    """(same, ambiguous) of every record: test_closest_segment.py's rule, a runner-up within REL and nothing else being what excuses"""
    is_nearest = (h["inst"] == r["inst"]) & (h["prim"] == r["prim"])
    if set_name in FLAT_SETS:
        touches = r["picked_t"] <= r["t"] + 8 * 2.0 ** -24 * r["mag"]
        return touches & ((r["level"] != 1) | is_nearest), r["runner_level"] <= r["t"] * (1 + REL)
    return r["picked_touches"] & ((r["touching"] != 1) | is_nearest), r["runner"] <= r["t"] * (1 + REL)


@pytest.mark.parametrize("scene_name", ["small", "small+1000", "teapot"])
def test_binary32_restatement_against_binary64(scene_name):
    """every set: t within the bound of the binary64 minimum over the six edge-against-triangle pairs; no feature undershoots
    (t32 >= t64 - K (1e-5 t + 1e-6 M) on every record); the identity rule of the module's docstring with at most 1 % excused"""
    sc, sets = cpu_results(scene_name)
    for name, (tris, h, quv, r) in sets.items():
        assert (h["inst"] >= 0).all() and (quv >= 0).all() and (quv <= 1).all() and not np.signbit(quv).any()
        t32 = h["t"].astype(np.float64)
        tol = cr.t_tolerance(r["t"], r["mag"])
        shallow = shallow_touches(sc, tris, r, h)
        err = np.abs(t32 - r["t"])
        plain = (err / tol)[~shallow].max(initial=0.0)
        sh = (err / (2.0 ** -12 * r["mag"]))[shallow].max(initial=0.0)
        under = ((r["t"] - t32) / tol).max()
        print("%s %s: worst t error %.3g of 1e-5 t + 1e-6 M; %d shallow touches, worst %.3g of 2^-12 M; worst undershoot %.3g" %
              (scene_name, name, plain, shallow.sum(), sh, under))
        assert (err <= t_bound(r, shallow)).all(), (name, plain, sh)
        assert (t32 >= r["t"] - K * tol).all(), (name, under)
        touches = r["t"] <= tol      # cut or touching: the key decides among residues; the reported triangle itself must be that near
        assert (np.abs(t32 - r["picked_t"]) <= t_bound(r, shallow))[touches].all(), name
        same, amb = identity(name, h, r)
        unexcused = np.nonzero(~same & ~amb & ~touches)[0]
        excused = (~same & ~touches).mean()
        print("%s %s: %.3f touch the surface; disagreeing %.4f, of them without a runner-up within REL: %s (records a runner-up could excuse: %.4f)" %
              (scene_name, name, touches.mean(), excused, unexcused.tolist(), (amb & ~touches).mean()))
        if (scene_name, name) not in IDENTITY_EXCLUDED:
            assert len(unexcused) == 0, (name, unexcused)
        assert excused <= 0.01, (name, excused)


def test_the_worst_committed_set_sets_k():
    """the set with the largest error found (a set of the GPU overlap test): its worst ratio is what K_MEASURED covers"""
    verts, idx, ranges, inst = small_scene(seed=WORST_SET["scene_seed"])
    sc = cr.Scene(verts, idx, ranges, inst)
    tris = triangle_sets(sc, WORST_SET["n"], seed=WORST_SET["set_seed"], closed=closed_of(inst))[WORST_SET["name"]]
    h, _, _ = tdr.brute32(sc, tris)
    r = tdr.brute64(sc, tris, picked=(h["inst"], h["prim"]))
    ratio = np.abs(h["t"].astype(np.float64) - r["t"]) / cr.t_tolerance(r["t"], r["mag"])
    print("worst t error %.3g of 1e-5 t + 1e-6 M (record %d)" % (ratio.max(), ratio.argmax()))
    assert K_MEASURED / 2 < ratio.max() <= K_MEASURED      # (the smallest power of two, and this set is why)
    assert (h["t"] >= r["t"] - K * cr.t_tolerance(r["t"], r["mag"])).all()


def test_binary64_decomposition_against_alternating_projections():
    """brute64's six edge-against-triangle pairs against altproj64 on the pair (record, its binary64 nearest triangle), every eighth record
    of every set: the projections reach a real pair, so brute64 <= altproj64 + tol always, on all 400 pairs.  The converse, altproj64 <=
    brute64 + tol, is asked of every set but the parallel and coplanar ones, cut records and the edge-parallel set included, 300 pairs,
    less the two of SLOW_PAIRS.  200 rounds reach the tolerance on 285 of them; the projections of the others creep (along the cut of two
    triangles that cut each other, along two parallel edges), so those pairs alone run 2000 rounds from the same start, which brings all
    but the two within 0.14 of the tolerance (the worst of the 285 is at 0.72)."""
    sc, sets = cpu_results("small")
    total = converse = 0
    for name, (tris, h, quv, r) in sets.items():
        i = np.arange(0, len(tris), 8)
        alt = tdr.altproj64(sc, tris, i, r["tri"][i])
        tol = cr.t_tolerance(r["t"][i], r["mag"][i])
        assert (r["t"][i] <= alt + tol).all(), name
        left = np.nonzero(alt > r["t"][i] + tol)[0]
        if len(left):
            alt[left] = tdr.altproj64(sc, tris, i[left], r["tri"][i[left]], rounds=2000)
        over = (alt - r["t"][i]) / tol
        print("%s: worst brute64 - altproj64 %.3g, worst altproj64 - brute64 %.3g (of the tolerance; %d pairs took 2000 rounds); records beyond it: %s" %
              (name, -over.min(), over.max(), len(left), i[over > 1].tolist()))
        assert (r["t"][i] <= alt + tol).all(), name
        if name not in ("parallel", "coplanar"):
            asked = ~np.isin(i, SLOW_PAIRS.get(name, ()))
            assert (over <= 1)[asked].all(), (name, i[asked & (over > 1)])
            converse += asked.sum()
        total += len(i)
    assert total >= 400 and converse >= 298


def test_point_identity_and_edge_property_of_the_restatement():
    """P0 == P1 == P2: brute32 equals closest_reference.brute32 of (P0, r_max) byte for byte, params 0; -0.0 against 0.0 compares equal.
    Edges: d2 never exceeds segment_reference.brute32's d2 of an edge record, and where a feature of steps 1 to 3 wins the record equals
    the best of the three edge records in (t, inst, prim, u, v)"""
    sc, sets = cpu_results("small")
    tris = np.concatenate([v[0][:100] for v in sets.values()])
    pts = tris.copy()
    pts[:, 4:7] = pts[:, 0:3]; pts[:, 8:11] = pts[:, 0:3]
    pts[::3, 3] = 0.4
    pts[5, 0], pts[5, 4], pts[5, 8] = F(0.0), F(-0.0), F(0.0)
    h, quv, _ = tdr.brute32(sc, pts)
    assert h.tobytes() == cr.brute32(sc, pts[:, :4]).tobytes() and (quv.view(np.uint32) == 0).all()
    assert (h["inst"] >= 0).mean() > 0.5 and (h["inst"] < 0).any()
    tris[::4, 3] = 0.5
    h, quv, d2 = tdr.brute32(sc, tris)
    h3, _, d23 = tdr.brute32(sc, tris, steps=3)
    edges = [sgr.brute32(sc, e)[0] for e in tdr.edge_records(tris)]
    match3, match = np.zeros(len(tris), bool), np.zeros(len(tris), bool)
    for e in edges:
        hit = e["inst"] >= 0
        assert (h["inst"][hit] >= 0).all() and (h["t"][hit] <= e["t"][hit]).all() and (h3["t"][hit] <= e["t"][hit]).all()
        rows = lambda x: x.view(np.uint8).reshape(len(x), -1)   # noqa: E731
        match3 |= hit & (rows(h3) == rows(e)).all(axis=1)
        match |= hit & (rows(h) == rows(e)).all(axis=1)
    # steps 1 to 3 alone ARE the best edge record: the record of an edge that attains the smallest key (several may, at d2 = 0), or a miss
    any_hit = np.logical_or.reduce([e["inst"] >= 0 for e in edges])
    assert np.array_equal(h3["inst"] >= 0, any_hit) and match3[any_hit].all()
    # the same triangle wins with the same d2 without steps 4 and 5: none of their features was strictly smaller
    early = (h["inst"] >= 0) & (d2 == d23) & (h["inst"] == h3["inst"]) & (h["prim"] == h3["prim"])
    assert match[early].all() and 0.3 < early.mean() < 1.0


def test_restatement_misses_radii_and_masks():
    sc, sets = cpu_results("small")
    tris, full, q_full, _ = sets["near"]
    d2 = tdr.brute32(sc, tris)[2]
    q = tris.copy(); q[:, 3] = full["t"]
    at, q_at, _ = tdr.brute32(sc, q)     # r_max = t: the smallest d2 is within reach exactly when the binary32 square of t does not round below it
    reach = F(full["t"] * full["t"]) >= d2      # (inclusive: sqrtf is exact on the many d2 whose root rounds to itself squared)
    assert np.array_equal(at["inst"] >= 0, reach) and 0.3 < reach.mean() and (F(full["t"] * full["t"]) == d2).any()
    assert at[reach].tobytes() == full[reach].tobytes() and q_at[reach].tobytes() == q_full[reach].tobytes()
    assert (at["inst"][~reach] == -1).all() and np.array_equal(at["t"][~reach], q[~reach, 3]) and (q_at[~reach] == 0).all()
    q[:, 3] = np.nextafter(full["t"], INF) * F(1.001)
    h, quv, _ = tdr.brute32(sc, q)
    assert h.tobytes() == full.tobytes() and quv.tobytes() == q_full.tobytes()
    far = full["t"] > 0
    q[:, 3] = full["t"] * F(0.99)
    m, quv, _ = tdr.brute32(sc, q)
    assert (m["inst"][far] == -1).all() and np.array_equal(m["t"], q[:, 3]) and (m["u"][far] == 0).all() and (quv[far] == 0).all() and far.mean() > 0.9
    q[:, 3] = 0.0
    z, _, _ = tdr.brute32(sc, q)
    assert (z["inst"][far] == -1).all() and (z["t"] == 0).all()
    assert (tdr.brute32(sc, tris, 0)[0]["inst"] == -1).all()
    for bit in (0x01, 0x10):
        one, _, _ = tdr.brute32(sc, tris, bit)
        assert ((sc.mask[one["inst"]] & bit) != 0).all() and (one["t"] >= full["t"]).all()
    others = 0xFF & ~sc.mask[full["inst"]]      # every bit but the nearest instance's own
    for cull in np.unique(others)[:4]:
        i = np.nonzero(others == cull)[0]
        ex, _, _ = tdr.brute32(sc, tris[i], int(cull))
        assert (ex["inst"] != full["inst"][i]).all() and (ex["t"] >= full["t"][i]).all()
    recs = invalid_records(tris)
    bad, quv, _ = tdr.brute32(sc, recs)
    assert (bad["inst"][:N_INVALID] == -1).all() and np.array_equal(bad["t"][:N_INVALID].view(np.uint32), recs[:N_INVALID, 3].view(np.uint32))
    assert (bad["u"][:N_INVALID] == 0).all() and (quv[:N_INVALID] == 0).all()
    assert (bad["inst"][[13, 14, 15]] >= 0).all() and not np.isnan(bad["t"][np.arange(len(bad)) != 10]).any()


def test_vertex_permutations():
    """the six orders of (P0, P1, P2): t within the bound, the same triangle where it is determined (no runner-up within REL, the surface
    not touched, one nearest triangle), and (qu, qv) naming the same point within 1e-4 of the query's longest edge (the flat sets aside)"""
    sc, sets = cpu_results("small")
    for name, (tris, h, quv, r) in sets.items():
        tris, h, quv = tris[:200], h[:200], quv[:200]
        r = {k: v[:200] for k, v in r.items()}
        P = tdr.vertices64(tris)
        longest = np.max([np.linalg.norm(P[j] - P[i], axis=1) for i, j in tdr.Q_EDGES], axis=0)
        point = P[0] + quv[:, 0:1].astype(np.float64) * (P[1] - P[0]) + quv[:, 1:2] * (P[2] - P[0])
        sure = ~identity(name, h, r)[1] & ~(r["t"] <= cr.t_tolerance(r["t"], r["mag"])) & ((r["level"] if name in FLAT_SETS else r["touching"]) == 1)
        worst = 0.0
        for perm in itertools.permutations(range(3)):
            pt = tris.copy()
            for k, src in enumerate(perm):
                pt[:, 4 * k:4 * k + 3] = tris[:, 4 * src:4 * src + 3]
            h2, q2, _ = tdr.brute32(sc, pt)
            shallow = shallow_touches(sc, tris, r, h) | shallow_touches(sc, tris, r, h2)
            assert (np.abs(h2["t"].astype(np.float64) - r["t"]) <= t_bound(r, shallow)).all(), (name, perm)
            same = (h2["inst"] == h["inst"]) & (h2["prim"] == h["prim"])
            assert same[sure].all(), (name, perm)
            if name not in FLAT_SETS:
                Q = [P[s] for s in perm]
                p2 = Q[0] + q2[:, 0:1].astype(np.float64) * (Q[1] - Q[0]) + q2[:, 1:2] * (Q[2] - Q[0])
                dp = np.linalg.norm(p2 - point, axis=1) / longest
                worst = max(worst, dp[same & sure].max(initial=0.0))
                assert (dp[same & sure] <= 1e-4).all(), (name, perm, dp[same & sure].max())
        print("%s: worst shift of the query's point over the permutations %.3g of the longest edge, %d records" % (name, worst, sure.sum()))


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
def test_small_scene_every_record_set(ctx):
    """every set of the CPU comparison plus records on vertices and edges and degenerate queries; r_max 0, t, 0.7 t, 1.5 t and inf; cull
    masks; invalid records; without attributes and without parameters; 1, 63, 65, 257 and 1500 records"""
    verts, idx, ranges, inst = small_scene(seed=51)
    sc, orc = load(ctx, verts, idx, ranges, inst)
    sets = triangle_sets(sc, 160, seed=52, closed=closed_of(inst))
    sets["features"] = feature_triangles(sc, 40, seed=53)
    for name, tris in sets.items():
        ref, _ = check(sc, orc, tris, gpu_triangles(ctx, tris), what=name)
        assert (ref["inst"] >= 0).all()
        q = tris.copy()
        k = np.arange(len(q)) % 4
        q[:, 3] = np.where(k == 0, 0.0, np.where(k == 1, ref["t"], np.where(k == 2, ref["t"] * F(0.7), ref["t"] * F(1.5))))
        ref2, _ = check(sc, orc, q, gpu_triangles(ctx, q), what=name + " radii")
        assert (ref2["inst"][(k == 2) & (ref["t"] > 0)] == -1).all() and (ref2["inst"][k == 3] >= 0).all()
        for cull in (0x01, 0x5A, 0x00):
            check(sc, orc, tris[:60], gpu_triangles(ctx, tris[:60], cull), cull, what="%s cull %#x" % (name, cull))
    bad = invalid_records(sets["across"])
    ref, _ = check(sc, orc, bad, gpu_triangles(ctx, bad), what="invalid records")
    assert (ref["inst"][:N_INVALID] == -1).all()
    h, a, quv = gpu_triangles(ctx, sets["near"], attributes=False, params=False)
    assert a is None and quv is None and h.tobytes() == tdr.brute32(sc, sets["near"])[0].tobytes()
    h, a, quv = gpu_triangles(ctx, sets["poke"], attributes=True, params=False)      # (the side words come from the workspace's parameters)
    check(sc, orc, sets["poke"], (h, a, None), what="attributes without parameters")
    h, a, quv = gpu_triangles(ctx, sets["poke"], attributes=False, params=True)
    check(sc, orc, sets["poke"], (h, None, quv), what="parameters without attributes")
    every = np.concatenate(list(sets.values()) * 2)[:1500]
    assert len(every) == 1500
    got = gpu_triangles(ctx, every)
    check(sc, orc, every, got, what="1500 records")
    for n in (1, 63, 65, 257):
        part = gpu_triangles(ctx, every[:n])
        assert all(x.tobytes() == y[:n].tobytes() for x, y in zip(part, got)), n


@pytest.mark.gpu
def test_point_identity_and_edge_property_on_the_device(ctx):
    """P0 == P1 == P2: the hits and attributes are closest_point_device's on the same context byte for byte, params 0.  Every record:
    t <= the t of closest_segment_device on each of its three edges, exactly, and an edge record that hits means the triangle hits"""
    import torch
    verts, idx, ranges, inst = small_scene(seed=55)
    sc, orc = load(ctx, verts, idx, ranges, inst)
    tris = np.concatenate(list(triangle_sets(sc, 220, seed=56, closed=closed_of(inst)).values()) + [feature_triangles(sc, 40, seed=57)])
    pts = tris.copy()
    pts[:, 4:7] = pts[:, 0:3]; pts[:, 8:11] = pts[:, 0:3]
    pts[::3, 3] = 0.4
    h, a, quv = gpu_triangles(ctx, pts)
    res = ctx.closest_point_device(torch.from_numpy(np.ascontiguousarray(pts[:, :4])).to("cuda:0"), attributes=True)
    torch.cuda.synchronize()
    hp, ap = res.numpy()
    assert h.tobytes() == hp.tobytes() and a.tobytes() == ap.tobytes() and (quv.view(np.uint32) == 0).all()
    assert (h["inst"] >= 0).mean() > 0.5 and (h["inst"] < 0).any()
    tris[::4, 3] = 0.5
    h, _, _ = gpu_triangles(ctx, tris, attributes=False)
    won = np.zeros(len(tris), bool)
    for e in tdr.edge_records(tris):
        he = ctx.closest_segment_device(torch.from_numpy(e).to("cuda:0")).numpy()[0]
        hit = he["inst"] >= 0
        assert (h["inst"][hit] >= 0).all() and (h["t"][hit] <= he["t"][hit]).all()
        won |= hit & (h["t"] == he["t"]) & (h["inst"] == he["inst"]) & (h["prim"] == he["prim"]) & (h["u"] == he["u"]) & (h["v"] == he["v"])
    assert 0.3 < won.mean() < 1.0      # (steps 1 to 3 win on most records, steps 4 and 5 on the rest)


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "1", "2", "3"])
def test_tree_independence(builder, monkeypatch):
    """the same records over every BLAS builder, host and device instance records with their refits, and a refitted BLAS: one brute force"""
    import torch
    from tests.test_blas_refit import deform, with_mesh
    verts, idx, ranges, inst = small_scene(seed=71)
    geom = types.SimpleNamespace(verts=verts, idx=idx, ranges=ranges)
    rng = np.random.default_rng(72)
    moved = inst.copy()
    moved["transform"][:, [3, 7, 11]] += rng.uniform(-0.3, 0.3, (len(inst), 3)).astype(F)
    sc0 = cr.Scene(verts, idx, ranges, inst)
    tris = np.concatenate(list(triangle_sets(sc0, 60, seed=73, closed=closed_of(inst)).values()) + [feature_triangles(sc0, 12, seed=74)])
    tris[::5, 3] = 0.5
    c = RtContext(0)
    try:
        use_builder(c, builder, monkeypatch)
        c.upload_geometry(verts, idx, ranges)
        for source in ("host", "device"):
            for recs, update in ((inst, False), (moved, True)):
                if source == "host":
                    c.set_instances(recs, update=update)
                else:
                    torch.cuda.synchronize()
                    c.set_instances_device(dev_inst(recs), update=update)
                sc, orc = cr.Scene(verts, idx, ranges, recs), oracle_scene(verts, idx, ranges, recs)
                if source == "host":
                    check(sc, orc, tris, gpu_triangles(c, tris, 0x5A), 0x5A, "%s records, update %d, builder %s, cull" % (source, update, builder))
                check(sc, orc, tris, gpu_triangles(c, tris), what="%s records, update %d, builder %s" % (source, update, builder))
        t = deform(geom, 0, amp=0.2)
        torch.cuda.synchronize()
        c.refit_blas_device(0, t)
        torch.cuda.synchronize()
        c.set_instances_device(dev_inst(inst))
        v2 = with_mesh(geom, verts, 0, t)
        check(cr.Scene(v2, idx, ranges, inst), oracle_scene(v2, idx, ranges, inst), tris, gpu_triangles(c, tris), what="refit, builder %s" % builder)
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small+1000", "small+10000", "cancel"])
def test_translated_and_cancelling_scenes(ctx, name):
    """the scene 1000 and 10000 units from the origin, and instances whose translation cancels their mesh's own offset (word 0 of the
    scale array): the bound's slack must cover the binary32 d2"""
    from tests.test_overlap_boxes import cancelling_scene
    verts, idx, ranges, inst = cancelling_scene() if name == "cancel" else small_scene(seed=81, offset=float(name.split("+")[1]))
    sc, orc = load(ctx, verts, idx, ranges, inst)
    sets = triangle_sets(sc, 120, seed=82, closed=closed_of(inst))
    sets["features"] = feature_triangles(sc, 30, seed=84)
    for sname, tris in sets.items():
        ref, _ = check(sc, orc, tris, gpu_triangles(ctx, tris), what="%s %s" % (name, sname))
        q = tris.copy(); q[:, 3] = ref["t"] * F(1.25)
        check(sc, orc, q, gpu_triangles(ctx, q, attributes=False), what="%s %s radii" % (name, sname))


@pytest.mark.gpu
def test_degenerate_triangles_and_a_singular_instance(ctx):
    """needles and zero-area triangles, and a singular (flattened) instance among them: byte-equal, no NaN t"""
    verts, idx, ranges = degenerate_soup(62)
    inst = placed_instances(12, 63, spacing=2.5, n_meshes=1)
    M = np.asarray(inst[3]["transform"], np.float64).reshape(3, 4)
    M[:, 2] = 0.0                                   # a flattened body: o2w is singular, its boxes do not prune
    inst[3]["transform"] = M.astype(F).reshape(12)
    with np.errstate(all="ignore"):                 # (the reference's inverse of the singular record is not finite, as the library's)
        sc, orc = load(ctx, verts, idx, ranges, inst)
    sets = triangle_sets(sc, 100, seed=64, closed=np.arange(len(inst)))
    sets["features"] = feature_triangles(sc, 30, seed=65)
    for name, tris in sets.items():
        h, a, quv = gpu_triangles(ctx, tris, attributes=False)
        assert not np.isnan(h["t"]).any() and not np.isnan(quv).any()
        check(sc, orc, tris, (h, None, quv), what="degenerate " + name)
        check(sc, orc, tris[:50], gpu_triangles(ctx, tris[:50]), what="degenerate %s with attributes" % name)
        q = tris[:50].copy(); q[:, 3] = 0.3
        check(sc, orc, q, gpu_triangles(ctx, q, attributes=False), what="degenerate %s radius" % name)


class TriangleQuery:
    """tests/stack_reference.py's model of this walk's descent: rule BOUND on test (i) of csrc/kernels_triangle.inc, the squared per-axis
    gap between the bounds of the three vertices and the child's box times the instance's scale squared, the smaller bound first; a
    child is entered while its bound does not exceed the search radius squared.  (Test (ii) only ever closes more boxes once a radius is
    finite: the model's `first` peaks are asserted for r_max = inf, its `full` peaks are upper bounds.)"""
    rule = "bound"

    def __init__(self, p, radius=np.inf, scale2=1.0):
        self.p, self.radius, self.scale2 = [[float(x) for x in v] for v in p], float(radius), float(scale2)

    def into(self, M, scale):
        f = lambda p: [M[a][0] * p[0] + M[a][1] * p[1] + M[a][2] * p[2] + M[a][3] for a in range(3)]   # noqa: E731
        return TriangleQuery([f(v) for v in self.p], self.radius, scale * scale)

    def test(self, lo, hi):
        d2 = 0.0
        for a in range(3):
            d = max(lo[a] - max(v[a] for v in self.p), min(v[a] for v in self.p) - hi[a], 0.0)
            d2 += d * d
        d2 *= self.scale2
        return not (d2 > self.radius * self.radius), d2


@pytest.mark.gpu
def test_the_spill_half_of_the_stack():
    """the corridor scene of tests/test_stack_spill.py: triangles off the ends of the deep corridors reach STACK2_LDS + 2 entries before
    the first triangle is tested, those at the ladder's foot stay in LDS, interleaved in one call; byte for byte"""
    from tests import test_stack_spill as tss
    small = tss.World(placed=tss.PLACED_SMALL)
    try:
        rays, tag, _ = tss.corridor_rays(tss.SMALL_TARGETS, 4, seed=16, placed=tss.PLACED_SMALL, inside=0.0)
        p0 = rays[:, 0:3] + F(2.0) * rays[:, 4:7]                      # 3 off an end of the row, inside the footprint
        rng = np.random.default_rng(17)
        p1 = p0 + F(1.5) * rays[:, 4:7] + rng.uniform(-0.5, 0.5, (len(p0), 3)).astype(F)
        p2 = p0 + F(0.7) * rays[:, 4:7] + rng.uniform(-0.5, 0.5, (len(p0), 3)).astype(F)
        r = np.where(np.arange(len(p0)) % 7 == 6, 4.0, np.inf)
        r[tag == -1] = 5.0
        r[tag == 0] = 6.0    # (the shallow end: a radius bounds the walk, so that the model's unpruned walk bounds it too)
        tris = records(p0, p1, p2, r)
        q = [TriangleQuery((x[0:3], x[4:7], x[8:11]), x[3]) for x in tris.astype(np.float64)]
        tss.premise(small.model, q, np.where(np.isinf(tris[:, 3]) | (tag == 0), tag, -2), (tss.S_TOP, tss.S_ROT0, tss.S_ROT1, tss.S_SHEAR), sample=3,
                    what="triangles")
        h, a, quv = gpu_triangles(small.ctx, tris)
        ref, q_ref, _ = tdr.brute32(small.sc, tris)
        assert h.tobytes() == ref.tobytes(), np.nonzero(h != ref)[0][:5]
        assert quv.tobytes() == q_ref.tobytes()
        assert (ref["inst"][tag == -1] == -1).all() and (ref["inst"][tag >= 0] == tag[tag >= 0]).all()
        kinds, _ = tdr.side_words(small.sc, tris, ref, q_ref)
        assert np.array_equal(a[:, 7].view(np.uint32), kinds)
    finally:
        small.ctx.close()


@pytest.mark.gpu
def test_consistency_with_the_overlap_query(ctx):
    """the same buffer through overlap_triangles_device(any=True) (it ignores word 3): every record that overlaps reports t within the
    touching bound, every record with t above the bound does not overlap.  The bound is K 1e-6 M, and K 2^-12 M where the query's plane
    is within SHALLOW radians of the reported triangle's"""
    import torch
    verts, idx, ranges, inst = small_scene(seed=91)
    sc, orc = load(ctx, verts, idx, ranges, inst)
    sets = triangle_sets(sc, 250, seed=92, closed=closed_of(inst))
    tris = np.concatenate([sets[k] for k in ("near", "across", "inside", "poke", "needles", "coplanar", "parallel")])
    src = dev(tris)
    res = ctx.closest_triangle_device(src)
    over = ctx.overlap_triangles_device(src, any=True)
    torch.cuda.synchronize()
    h, cnt = res.numpy()[0], over.count.cpu().numpy()
    assert (h["inst"] >= 0).all()
    first = np.concatenate([[0], np.cumsum(np.bincount(sc.inst, minlength=len(sc.mask)))])
    tri = first[h["inst"]] + h["prim"]
    mag = np.maximum(np.abs(tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]).max(axis=1), np.abs(np.concatenate([sc.A[tri], sc.B[tri], sc.C[tri]], axis=1)).max(axis=1))
    bound = np.where(plane_sines(sc, tris, tri) >= SHALLOW, K * 1e-6 * mag, K * 2.0 ** -12 * mag)
    t = h["t"].astype(np.float64)
    print("overlapping %.3f; worst t of an overlapping record %.3g of its bound" % ((cnt > 0).mean(), (t / bound)[cnt > 0].max()))
    assert 0.2 < (cnt > 0).mean() < 0.9
    assert (t[cnt > 0] <= bound[cnt > 0]).all(), np.nonzero((cnt > 0) & (t > bound))[0][:5]
    assert (cnt[t > bound] == 0).all()


@pytest.mark.gpu
def test_plumbing(ctx):
    """host form = device form; counting; out= reuse; stream order behind a slow queue on a side stream; a shading call queued between
    two triangle queries; n == 0; device tensors through triangle_records"""
    import torch
    from tests.test_ray_query import mixed_rays
    sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
    g = sp.geom
    sc, orc = load(ctx, g.verts, g.idx, g.ranges, sp.instances)
    ctx.set_uniforms(sp.uniforms)
    tris = np.concatenate(list(triangle_sets(sc, 12, seed=102, closed=np.arange(len(sp.instances))).values()))
    tris[::4, 3] = 0.5
    ref, q_ref = check(sc, orc, tris, gpu_triangles(ctx, tris), what="device form")
    hh, st = ctx.closest_triangle(tris)
    assert hh.tobytes() == ref.tobytes() and st.node_visits == 0 and st.bvh_node_bytes > 0
    hc, q_host, st = ctx.closest_triangle(tris, params=True, counting=True)
    assert hc.tobytes() == ref.tobytes() and q_host.tobytes() == q_ref.tobytes() and st.node_visits > 0 and st.tri_tests > 0
    assert ctx.closest_triangle(tris, cull_mask=0)[0]["inst"].max() == -1
    # out= reuse
    src = dev(tris)
    n = len(tris)
    hits = torch.empty((n, 5), dtype=torch.int32, device="cuda:0"); attr = torch.empty((n, 8), dtype=torch.int32, device="cuda:0")
    par = torch.empty((n, 2), dtype=torch.float32, device="cuda:0")
    res = ctx.closest_triangle_device(src, attributes=True, params=True, out=(hits, attr, par))
    assert res.hits.data_ptr() == hits.data_ptr() and res.attr.data_ptr() == attr.data_ptr() and res.quv.data_ptr() == par.data_ptr()
    assert res.numpy()[0].tobytes() == ref.tobytes() and res.quv.cpu().numpy().tobytes() == q_ref.tobytes()
    with pytest.raises(ValueError):
        ctx.closest_triangle_device(src, out=(hits[:-1], None))
    with pytest.raises(ValueError):
        ctx.closest_triangle_device(src, params=True, out=(hits, None, par[:-1]))
    # stream order
    rays = torch.from_numpy(mixed_rays(n, seed=103)).to("cuda:0")
    closest = ctx.intersect_device(rays).numpy()[0]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = slow_queue(torch, 12)
        p = (src + (a[0, 0] != a[0, 0]).to(torch.float32) * 0).contiguous()   # made behind the queue, on the side stream
        r1 = ctx.closest_triangle_device(p, attributes=True, params=True, stream=side)
        q1 = ctx.intersect_device(rays, stream=side)
        img = ctx.shade_rays_device(rays, stream=side)                         # a shading call between two triangle queries
        r2 = ctx.closest_triangle_device(p, stream=side)
        p.zero_()                                                             # overwritten right after the calls
        h1, h2, hq, q1c = r1.hits.clone(), r2.hits.clone(), q1.hits.clone(), r1.quv.clone()
    side.synchronize()
    assert img is not None and img[1] is not None and tuple(img[1].shape) == (rays.shape[0], 4)
    for hcopy in (h1, h2):
        assert hcopy.cpu().numpy().view(HIT_DTYPE).reshape(-1).tobytes() == ref.tobytes()
    assert q1c.cpu().numpy().tobytes() == q_ref.tobytes()
    assert hq.cpu().numpy().view(HIT_DTYPE).reshape(-1).tobytes() == closest.tobytes()
    # n == 0
    e = ctx.closest_triangle_device(torch.empty((0, 12), dtype=torch.float32, device="cuda:0"), attributes=True, params=True)
    assert e.hits.shape == (0, 5) and e.attr.shape == (0, 8) and e.quv.shape == (0, 2)
    assert len(ctx.closest_triangle(np.zeros((0, 12), F))[0]) == 0
    # device tensors through triangle_records
    v = torch.stack([src[:, 0:3], src[:, 4:7], src[:, 8:11]], dim=1).reshape(-1, 3)
    rec = api.triangle_records(v, torch.arange(3 * n, device="cuda:0").reshape(-1, 3), r_max=src[:, 3])
    assert rec.is_cuda and torch.equal(rec, src)


def _raw(c, n, tris, cull, hits, attr, par):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_closest_triangle_device(c.h, n, p(tris), cull, p(hits), p(attr), p(par), None)


@pytest.mark.gpu
def test_error_statuses():
    import torch
    verts, idx, ranges, inst = small_scene(seed=121)
    sc = cr.Scene(verts, idx, ranges, inst)
    tris_np = triangle_sets(sc, 100, seed=122, closed=closed_of(inst))["near"]
    ref, _, _ = tdr.brute32(sc, tris_np)
    tris = dev(tris_np)
    n = tris.shape[0]
    hits = torch.empty((n + 1, 5), dtype=torch.int32, device="cuda:0")
    attr = torch.empty((n + 1, 8), dtype=torch.int32, device="cuda:0")
    par = torch.empty((n + 1, 2), dtype=torch.float32, device="cuda:0")
    S_, H_, A_, P_ = tris.data_ptr(), hits.data_ptr(), attr.data_ptr(), par.data_ptr()
    c = RtContext(0)

    def err(args, code, text):
        assert _raw(c, *args) == code, args
        msg = c.L.rt_last_error(c.h).decode()
        assert text in msg, (args, msg)

    def ok():
        assert c.closest_triangle_device(tris).numpy()[0].tobytes() == ref.tobytes()

    try:
        err((n, S_, 0xFF, H_, 0, 0), RT_ERR_NOT_READY, "")   # no geometry
        c.upload_geometry(verts, idx, ranges)
        err((n, S_, 0xFF, H_, 0, 0), RT_ERR_NOT_READY, "")   # no TLAS
        c.set_instances(inst)
        ok()
        bad = [((0xFFFFFF00, S_, 0xFF, H_, 0, 0), "too many triangles"), ((n, S_, 0x100, H_, 0, 0), "cull_mask"), ((n, 0, 0xFF, H_, 0, 0), "null triangle/hit pointers"),
               ((n, S_, 0xFF, 0, 0, 0), "null triangle/hit pointers"), ((n, S_ + 4, 0xFF, H_, 0, 0), "aligned"), ((n, S_, 0xFF, H_ + 2, 0, 0), "aligned"),
               ((n, S_, 0xFF, H_, A_ + 4, 0), "aligned"), ((n, S_, 0xFF, H_, 0, P_ + 2), "aligned")]
        host_buf = np.zeros((n + 1, 12), F)
        pinned = torch.zeros((n, 12), dtype=torch.float32).pin_memory()
        for ptr in ((host_buf.ctypes.data + 15) & ~15, pinned.data_ptr()):   # (16-byte aligned: only the memory kind is wrong)
            bad += [((n, ptr, 0xFF, H_, 0, 0), "device memory of the context's GPU"), ((n, S_, 0xFF, ptr, 0, 0), "device memory of the context's GPU"),
                    ((n, S_, 0xFF, H_, ptr, 0), "device memory of the context's GPU"), ((n, S_, 0xFF, H_, 0, ptr), "device memory of the context's GPU")]
        for args, text in bad:
            err(args, RT_ERR_INVALID_ARGUMENT, text)
        ok()
        err((n, S_, 0xFF, H_, 0, P_ + 4), 0, "")             # the parameters need 4-byte alignment only
        out = np.zeros(n, HIT_DTYPE)
        assert c.L.rt_closest_triangle(c.h, n, None, 0xFF, out.ctypes.data_as(ctypes.c_void_p), None, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_closest_triangle(c.h, n, tris_np.ctypes.data_as(ctypes.c_void_p), 0x100, out.ctypes.data_as(ctypes.c_void_p), None, 0, None) == RT_ERR_INVALID_ARGUMENT
        ok()
        assert _raw(c, 0, 0, 0xFF, 0, 0, 0) == 0   # n == 0 enqueues nothing and needs no pointers
        with pytest.raises(ValueError):
            c.closest_triangle_device(tris.cpu())
        with pytest.raises(ValueError):
            c.closest_triangle_device(torch.zeros((4, 8), dtype=torch.float32, device="cuda:0"))
        with pytest.raises(RtError) as e:
            c.closest_triangle_device(tris, cull_mask=0x1FF)
        assert e.value.code == RT_ERR_INVALID_ARGUMENT
        ok()
    finally:
        c.close()
    # trace_variant != 0 (alt library only: the product refuses the parameter itself)
    a = RtContext(0, variant="alt")
    try:
        a.set_param("blas_builder", 0)
        a.set_param("trace_variant", 1)
        a.upload_geometry(verts, idx, ranges)
        a.set_instances(inst)
        c = a
        err((n, S_, 0xFF, H_, 0, 0), RT_ERR_INVALID_ARGUMENT, "trace_variant 0")
        a.set_param("trace_variant", 0)
        a.set_instances(inst)
        ok()
    finally:
        a.close()
