"""rt_closest_segment_device / rt_closest_segment: the nearest pair of every segment and the scene's surface.

tests/segment_reference.py holds the two references: brute32, the canonical binary32 feature sequence and key of include/rt_api.h and
DESIGN.md §5 "Closest points of segments" restated in numpy over every triangle, and brute64, the binary64 point-to-triangle distance
minimised over the segment's parameter by a ternary search.  The CPU part holds brute32 to brute64; the GPU part holds the library to
brute32 byte for byte: hits, parameters, attributes (against the oracle's hit_attributes of the returned records) and side words, under
every tree the library can build, far from the origin, on degenerate geometry, in the spill half of the stack, against the sphere
sweep, and the plumbing of a device query.

Identity against binary64 is test_closest_point.py's rule (the reported triangle touches the binary64 nearest point and is the binary64
triangle where only one touches it; at most 1 % of the records excused by a runner-up within REL) for the records whose binary64
distance exceeds the tolerance.  A record whose binary64 distance is zero within the tolerance pierces or touches the surface, often
several triangles of it (a closed mesh is entered and left): there the contract lets the key decide among residues, so the test asks
instead that the reported triangle's own binary64 distance to the segment be within the bound."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import closest_reference as cr
from tests import scenes
from tests import segment_reference as sgr
from tests.query_reference import REL
from tests.test_closest_point import degenerate_soup, scene_box, small_scene, surface_points, teapot_scene
from tests.test_ray_query import PATHS, dev_inst, slow_queue
from tests.test_ray_query_oracle import oracle_scene, placed_instances, use_builder
from vulkan_raytracing_amd import RtContext, api
from vulkan_raytracing_amd.api import HIT_DTYPE, RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
INF = np.float32(np.inf)
# |t32 - t64| <= K (1e-5 t + 1e-6 M): the smallest power of two that holds on every committed set is K_MEASURED (test 3 prints the worst
# ratio of every set); the bound asserted is four times it.  Shallow crossings (below) are held to K sqrt(2^-24) M.
K_MEASURED = 0.25        # (the worst committed set, edge-parallel segments on the small scene, reaches 0.142 of the plain bound)
K = 4.0 * K_MEASURED
SHALLOW = 2.0 ** -8      # radians between the segment and the plane of a triangle it touches


# ---- scenes and record sets ---------------------------------------------------------------------------------------------------

def records(p0, p1, r=np.inf):
    return api.capsule_records(np.asarray(p0, np.float64), np.asarray(p1, np.float64), r)


def unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def inside_points(sc, n, rng, closed):
    """points inside the world image of instances of the closed mesh: between the mean of the instance's vertices and a random point of
    a random triangle of it, 20 to 70 % of the way (generic positions: the centre itself is equidistant from many faces)"""
    first = np.concatenate([[0], np.cumsum(np.bincount(sc.inst, minlength=len(sc.mask)))])
    ii = closed[rng.integers(0, len(closed), n)]
    out = np.zeros((n, 3))
    for j, i in enumerate(ii):
        P = np.concatenate([sc.A[first[i]:first[i + 1]], sc.B[first[i]:first[i + 1]], sc.C[first[i]:first[i + 1]]])
        k = rng.integers(first[i], first[i + 1])
        w = rng.dirichlet((1.0, 1.0, 1.0))
        c = P.mean(axis=0)
        out[j] = c + rng.uniform(0.2, 0.7) * (w[0] * sc.A[k] + w[1] * sc.B[k] + w[2] * sc.C[k] - c)
    return out


def segment_sets(sc, n, seed, closed):
    """short segments near the surface; segments across the scene (many pierce); segments inside closed meshes; segments parallel to an
    edge of a triangle; segments in a triangle's plane, outside it and across it; segments with one or two zero direction components.
    r_max = inf"""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(sc)
    c, diag = (lo + hi) / 2, np.linalg.norm(hi - lo)
    sets = {}
    p = surface_points(sc, n, rng, 0.02 * diag)
    sets["short"] = records(p, p + unit(rng, n) * rng.uniform(0.001, 0.03, (n, 1)) * diag)
    sets["across"] = records(c + rng.uniform(-0.55, 0.55, (n, 3)) * (hi - lo), c + rng.uniform(-0.55, 0.55, (n, 3)) * (hi - lo))
    p, q = inside_points(sc, n, rng, closed), inside_points(sc, n, rng, closed)
    sets["inside"] = records(p, np.where((np.arange(n) % 2 == 0)[:, None], p + 0.3 * (q - p) / np.maximum(1.0, np.linalg.norm(q - p, axis=1, keepdims=True)), p + unit(rng, n) * 0.02))
    k = rng.integers(0, sc.n_tris, n)
    A, B, C = sc.A[k], sc.B[k], sc.C[k]
    e0 = np.where((k % 3 == 0)[:, None], A, np.where((k % 3 == 1)[:, None], B, C))
    e1 = np.where((k % 3 == 0)[:, None], B, np.where((k % 3 == 1)[:, None], C, A))
    off = unit(rng, n) * rng.uniform(0.0, 0.01, (n, 1)) * diag
    a, b = rng.uniform(-0.3, 0.6, (n, 1)), rng.uniform(0.4, 1.3, (n, 1))
    sets["edge-parallel"] = records(e0 + a * (e1 - e0) + off, e0 + b * (e1 - e0) + off)
    # in the plane: barycentrics (u, v) of both endpoints; outside: both beyond the edge BC; across: one inside, one anywhere around
    u0, v0 = rng.uniform(0.1, 0.4, (n, 1)), rng.uniform(0.1, 0.4, (n, 1))
    u1, v1 = rng.uniform(-1.5, 2.0, (n, 1)), rng.uniform(-1.5, 2.0, (n, 1))
    outside = (np.arange(n) % 2 == 0)[:, None]
    u0, v0 = np.where(outside, rng.uniform(0.7, 1.5, (n, 1)), u0), np.where(outside, rng.uniform(0.7, 1.5, (n, 1)), v0)
    u1, v1 = np.where(outside, rng.uniform(0.7, 2.5, (n, 1)), u1), np.where(outside, rng.uniform(0.7, 2.5, (n, 1)), v1)
    sets["in-plane"] = records(A + u0 * (B - A) + v0 * (C - A), A + u1 * (B - A) + v1 * (C - A))
    p = surface_points(sc, n, rng, 0.03 * diag)
    d = unit(rng, n) * rng.uniform(0.01, 0.2, (n, 1)) * diag
    zero = np.arange(n) % 6
    for ax in range(3):
        d[:, ax] = np.where((zero == ax) | (zero == 3 + ax) | (zero == 3 + (ax + 1) % 3), 0.0, d[:, ax])
    sets["axis"] = records(p, p.astype(np.float32).astype(np.float64) + d)
    return sets


FLAT_SETS = ("edge-parallel", "in-plane")     # the distance is flat in s: s is left out of the swap comparison


def feature_segments(sc, n, seed):
    """an endpoint exactly on a world vertex, an endpoint (to binary32 rounding) on an edge, and segments from vertex to vertex"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, sc.n_tris, n)
    on_v = np.where((k % 3 == 0)[:, None], sc.A[k], np.where((k % 3 == 1)[:, None], sc.B[k], sc.C[k]))
    s = rng.uniform(size=(n, 1))
    on_e = sc.A[k] + s * (sc.B[k] - sc.A[k])
    far = on_v + unit(rng, n) * rng.uniform(0.05, 1.0, (n, 1))
    k2 = rng.integers(0, sc.n_tris, n)
    return np.concatenate([records(on_v, far), records(far, on_e), records(on_v, sc.C[k2])])


def invalid_records(s):
    """records the contract answers with the miss form: NaN / inf in each endpoint, r_max of -1, NaN and -inf; then valid ones"""
    q = np.array(s[:14], np.float32).copy()
    q[0, 0] = np.nan; q[1, 1] = np.inf; q[2, 2] = -np.inf; q[3, 4] = np.nan; q[4, 5] = -np.inf; q[5, 6] = np.inf
    q[6, 3] = -1.0; q[7, 3] = np.nan; q[8, 3] = -np.inf
    q[9, 3] = np.float32(-0.0); q[10, 3] = 0.0; q[11, 3] = 3e38; q[12, 3] = 1e-30; q[13, 7] = np.nan   # (word 7 is ignored)
    return q


N_INVALID = 9


def dev(s):
    import torch
    return torch.from_numpy(np.ascontiguousarray(s, np.float32).reshape(-1, 8)).to("cuda:0")


def gpu_segments(ctx, segs, cull=0xFF, attributes=True, params=True):
    import torch
    res = ctx.closest_segment_device(dev(segs), cull_mask=cull, attributes=attributes, params=params)
    torch.cuda.synchronize()
    h, a = res.numpy()
    return h, a, (res.s.cpu().numpy() if res.s is not None else None)


def check(sc, orc, segs, got, cull=0xFF, what=""):
    """the GPU's (hits, attributes, s) against brute32 byte for byte; attributes against orc.hit_attributes of the returned records and
    the restated side words"""
    h, a, s = got
    ref, s_ref = sgr.brute32(sc, segs, cull)
    if h.tobytes() != ref.tobytes():
        bad = np.nonzero((h.view(np.uint8).reshape(len(h), -1) != ref.view(np.uint8).reshape(len(h), -1)).any(axis=1))[0]
        raise AssertionError("%s: %d records differ from the brute force, first %d: segment %s gpu %s reference %s" %
                             (what, len(bad), bad[0], np.asarray(segs).reshape(-1, 8)[bad[0]], h[bad[0]], ref[bad[0]]))
    if s is not None:
        assert s.tobytes() == s_ref.tobytes(), (what, np.nonzero(s.view(np.uint32) != s_ref.view(np.uint32))[0][:5])
    r_max = np.asarray(segs, np.float32).reshape(-1, 8)[:, 3]
    assert not np.isnan(h["t"][~np.isnan(r_max)]).any(), what
    if a is not None:
        kinds, _ = sgr.side_words(sc, segs, ref, s_ref)
        assert np.array_equal(a[:, 7].view(np.uint32), kinds), what
        o = orc.hit_attributes(np.ascontiguousarray(h))
        f = a.view(np.float32)
        assert np.array_equal(f[:, 0:3].view(np.uint32), o[:, 0:3].view(np.uint32)), what
        assert np.array_equal(f[:, 4:7].view(np.uint32), o[:, 3:6].view(np.uint32)), what
        assert np.array_equal(a[:, 3], o[:, 6].astype(np.int32)), what
        miss = h["inst"] < 0
        assert (a[miss, 0:3] == 0).all() and (a[miss, 4:7] == 0).all() and (a[miss, 7] == 0).all() and (a[miss, 3] == -1).all(), what
    return ref, s_ref


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_exports_abi_and_null_context():
    assert "rt_closest_segment_device" in api.EXPORTS and "rt_closest_segment" in api.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^int rt_closest_segment_device\(rt_ctx\* ctx, size_t n, const void\* d_segs8, uint32_t cull_mask,\s+void\* d_hits, void\* d_attr, "
                     r"void\* d_params, void\* hip_stream\);", hdr, re.M)
    assert re.search(r"^int rt_closest_segment\(rt_ctx\* ctx, size_t n, const float\* segs8_host, uint32_t cull_mask,\s+rt_hit\* out_host, "
                     r"float\* params_host, int counting, rt_stats\* stats\);", hdr, re.M)
    assert "rounding residue" in hdr and "the key decides" in hdr
    L = api.lib()
    assert hasattr(L, "rt_closest_segment_device") and hasattr(L, "rt_closest_segment") and L.rt_abi_version() == 7
    assert L.rt_closest_segment_device(None, 0, None, 0xFF, None, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_closest_segment_device(None, 64, None, 0xFF, None, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_closest_segment(None, 0, None, 0xFF, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert hasattr(RtContext, "closest_segment_device") and hasattr(RtContext, "closest_segment") and hasattr(api, "capsule_records")
    rec = api.capsule_records([[1, 2, 3]], [[4, 5, 6]], 7.0)
    assert rec.dtype == np.float32 and rec.tolist() == [[1, 2, 3, 7, 4, 5, 6, 0]]


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_segment_kernels_keep_the_record_level_budget(target):
    """k_closest_segment and its counting form keep the record-level walks' budget (>= 4 waves per SIMD, scratch <= 32 bytes, no
    spills); k_segment_side uses no scratch and spills nothing; one of each in both libraries"""
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    walk = [(n, r) for n, r in kernels.items() if "k_closest_segment" in n]
    side = [(n, r) for n, r in kernels.items() if "k_segment_side" in n]
    assert len(walk) == 2 and len(side) == 1, "\n".join(kernels)
    assert sum("k_closest_segment_count" in n for n, _ in walk) == 1
    for name, r in walk:
        assert int(r["Occupancy"]) >= 4 and int(r["ScratchSize"]) <= 32 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
    for name, r in side:
        assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)


def cpu_scene(scene_name):
    verts, idx, ranges, inst = teapot_scene() if scene_name == "teapot" else small_scene(offset=1000.0 if "+" in scene_name else 0.0)
    sc = cr.Scene(verts, idx, ranges, inst)
    closed = np.arange(len(inst)) if scene_name == "teapot" else np.nonzero(inst["mesh"] == 0)[0]
    return sc, closed


def shallow_crossings(sc, segs, r, picked):
    """(n,) bool: the segment lies within SHALLOW radians of the plane of a triangle it touches (its binary64 distance to that triangle
    is within the plain tolerance): the binary64 nearest triangle or the reported one"""
    sg = np.asarray(segs, np.float64).reshape(-1, 8)
    d = sg[:, 4:7] - sg[:, 0:3]
    first = np.concatenate([[0], np.cumsum(np.bincount(sc.inst, minlength=len(sc.mask)))])
    tol = cr.t_tolerance(r["t"], r["mag"])
    out = np.zeros(len(sg), bool)
    for tri, dist in ((r["tri"], r["t"]), (first[np.clip(picked["inst"], 0, None)] + picked["prim"], r["picked_t"])):
        tri = np.clip(tri, 0, sc.n_tris - 1)
        N = np.cross(sc.B[tri] - sc.A[tri], sc.C[tri] - sc.A[tri])
        with np.errstate(all="ignore"):
            sin = np.abs((N * d).sum(-1)) / (np.linalg.norm(N, axis=1) * np.linalg.norm(d, axis=1))
        out |= (dist <= tol) & ~(sin >= SHALLOW)
    return out


_CPU = {}


def cpu_results(scene_name):
    """{set: (segments, brute32 hits, brute32 s, brute64 dict)} of a CPU scene, computed once"""
    if scene_name not in _CPU:
        sc, closed = cpu_scene(scene_name)
        out = {}
        for name, segs in segment_sets(sc, 60 if scene_name == "teapot" else 400, seed=231, closed=closed).items():
            h, s = sgr.brute32(sc, segs)
            out[name] = (segs, h, s, sgr.brute64(sc, segs, picked=(h["inst"], h["prim"])))
        _CPU[scene_name] = (sc, out)
    return _CPU[scene_name]


def t_bound(r, shallow):
    """the bound on |t32 - t64|: K (1e-5 t + 1e-6 M), for shallow crossings K sqrt(2^-24) M"""
    return np.where(shallow, K * 2.0 ** -12 * r["mag"], K * cr.t_tolerance(r["t"], r["mag"]))


def identity(set_name, h, r):
    """(same, ambiguous) of every record.  same: the reported triangle touches the binary64 nearest point and is the binary64 triangle
    where only one touches it; ambiguous: a runner-up that does not touch it lies within REL.  Where the nearest pair is a continuum by
    construction (FLAT_SETS) there is no one nearest point: "touches" is then "is as near as the nearest within 8 x 2^-24 M"."""
    is_nearest = (h["inst"] == r["inst"]) & (h["prim"] == r["prim"])
    if set_name in FLAT_SETS:
        touches = r["picked_t"] <= r["t"] + 8 * 2.0 ** -24 * r["mag"]
        return touches & ((r["level"] != 1) | is_nearest), r["runner_level"] <= r["t"] * (1 + REL)
    return r["picked_touches"] & ((r["touching"] != 1) | is_nearest), r["runner"] <= r["t"] * (1 + REL)


@pytest.mark.parametrize("scene_name", ["small", "small+1000", "teapot"])
def test_binary32_restatement_against_binary64(scene_name):
    """every set: t within the bound of the binary64 minimum over s; no feature undershoots (t32 >= t64 - K (1e-5 t + 1e-6 M) on every
    record, shallow crossings and the in-plane sets included); the identity rule of the module's docstring with at most 1 % excused"""
    sc, sets = cpu_results(scene_name)
    for name, (segs, h, s, r) in sets.items():
        assert (h["inst"] >= 0).all() and (s >= 0).all() and (s <= 1).all()
        t32 = h["t"].astype(np.float64)
        tol = cr.t_tolerance(r["t"], r["mag"])
        shallow = shallow_crossings(sc, segs, r, h)
        err = np.abs(t32 - r["t"])
        plain = (err / tol)[~shallow].max(initial=0.0)
        sh = (err / (2.0 ** -12 * r["mag"]))[shallow].max(initial=0.0)
        under = ((r["t"] - t32) / tol).max()
        print("%s %s: worst t error %.3g of 1e-5 t + 1e-6 M; %d shallow crossings, worst %.3g of sqrt(2^-24) M; worst undershoot %.3g" %
              (scene_name, name, plain, shallow.sum(), sh, under))
        assert (err <= t_bound(r, shallow)).all(), (name, plain, sh)
        assert (t32 >= r["t"] - K * tol).all(), (name, under)
        touches = r["t"] <= tol      # pierced or touching: the key decides among residues; the reported triangle itself must be that near
        assert (np.abs(t32 - r["picked_t"]) <= t_bound(r, shallow))[touches].all(), name
        same, amb = identity(name, h, r)
        assert same[~amb & ~touches].all(), name
        excused = (~same & ~touches).mean()
        print("%s %s: %.3f touch the surface; excused %.4f (records a runner-up could excuse: %.4f)" % (scene_name, name, touches.mean(), excused, (amb & ~touches).mean()))
        assert excused <= 0.01, (name, excused)


def test_point_identity_of_the_restatement():
    """P0 == P1: brute32 equals closest_reference.brute32 of (P0, r_max) byte for byte, s = 0; -0.0 against 0.0 compares equal"""
    sc, sets = cpu_results("small")
    segs = np.concatenate([v[0][:150] for v in sets.values()])
    segs[:, 4:7] = segs[:, 0:3]
    segs[::3, 3] = 0.4
    segs[5, 0], segs[5, 4] = np.float32(0.0), np.float32(-0.0)
    h, s = sgr.brute32(sc, segs)
    assert h.tobytes() == cr.brute32(sc, segs[:, :4]).tobytes() and (s == 0).all() and not np.signbit(s).any()
    assert (h["inst"] >= 0).mean() > 0.5 and (h["inst"] < 0).any()


def test_restatement_misses_radii_and_masks():
    sc, sets = cpu_results("small")
    segs, full, s_full, _ = sets["short"]
    q = segs.copy(); q[:, 3] = full["t"]
    at, _ = sgr.brute32(sc, q)     # r_max = t: d2 <= r_max * r_max holds unless the square rounds below d2
    assert (at["inst"] >= 0).mean() > 0.3
    q[:, 3] = np.nextafter(full["t"], INF) * np.float32(1.001)
    h, s = sgr.brute32(sc, q)
    assert h.tobytes() == full.tobytes() and s.tobytes() == s_full.tobytes()
    far = full["t"] > 0
    q[:, 3] = full["t"] * np.float32(0.99)
    m, s = sgr.brute32(sc, q)
    assert (m["inst"][far] == -1).all() and np.array_equal(m["t"], q[:, 3]) and (m["u"][far] == 0).all() and (s[far] == 0).all() and far.mean() > 0.9
    assert (sgr.brute32(sc, segs, 0)[0]["inst"] == -1).all()
    for bit in (0x01, 0x10):
        one, _ = sgr.brute32(sc, segs, bit)
        assert ((sc.mask[one["inst"]] & bit) != 0).all() and (one["t"] >= full["t"]).all()
    recs = invalid_records(segs)
    bad, s = sgr.brute32(sc, recs)
    assert (bad["inst"][:N_INVALID] == -1).all() and np.array_equal(bad["t"][:N_INVALID].view(np.uint32), recs[:N_INVALID, 3].view(np.uint32))
    assert (bad["u"][:N_INVALID] == 0).all() and (s[:N_INVALID] == 0).all()
    assert (bad["inst"][[11, 13]] >= 0).all() and not np.isnan(bad["t"][np.arange(len(bad)) != 7]).any()


def test_swapped_endpoints():
    """P0 and P1 exchanged: t within the bound, the same triangle where no runner-up is within REL and the surface is not touched,
    s -> 1 - s within 1e-4 (the parallel and in-plane sets aside, and where the triangle is the same)"""
    sc, sets = cpu_results("small")
    for name, (segs, h, s, r) in sets.items():
        sw = segs.copy()
        sw[:, 0:3], sw[:, 4:7] = segs[:, 4:7], segs[:, 0:3]
        h2, s2 = sgr.brute32(sc, sw)
        shallow = shallow_crossings(sc, segs, r, h) | shallow_crossings(sc, segs, r, h2)
        assert (np.abs(h2["t"].astype(np.float64) - r["t"]) <= t_bound(r, shallow)).all(), name
        same = (h2["inst"] == h["inst"]) & (h2["prim"] == h["prim"])
        sure = ~identity(name, h, r)[1] & ~(r["t"] <= cr.t_tolerance(r["t"], r["mag"])) & ((r["level"] if name in FLAT_SETS else r["touching"]) == 1)
        assert same[sure].all(), name
        if name not in FLAT_SETS:
            ds = np.abs(s2.astype(np.float64) - (1.0 - s.astype(np.float64)))
            print("%s: worst |s' - (1 - s)| %.3g over %d records" % (name, ds[same & sure].max(initial=0.0), (same & sure).sum()))
            assert (ds[same & sure] <= 1e-4).all(), (name, ds[same & sure].max())


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
    """every set of the CPU comparison plus records on vertices and edges; r_max 0, t, 0.7 t, 1.5 t and inf; cull masks 0xFF, single
    bits, 0; invalid records; without attributes and without parameters; 1, 63, 65, 257 and 3000 records"""
    verts, idx, ranges, inst = small_scene(seed=51)
    sc, orc = load(ctx, verts, idx, ranges, inst)
    sets = segment_sets(sc, 500, seed=52, closed=np.nonzero(inst["mesh"] == 0)[0])
    sets["features"] = feature_segments(sc, 200, seed=53)
    for name, segs in sets.items():
        ref, _ = check(sc, orc, segs, gpu_segments(ctx, segs), what=name)
        assert (ref["inst"] >= 0).all()
        q = segs.copy()
        k = np.arange(len(q)) % 4
        q[:, 3] = np.where(k == 0, 0.0, np.where(k == 1, ref["t"], np.where(k == 2, ref["t"] * np.float32(0.7), ref["t"] * np.float32(1.5))))
        ref2, _ = check(sc, orc, q, gpu_segments(ctx, q), what=name + " radii")
        assert (ref2["inst"][(k == 2) & (ref["t"] > 0)] == -1).all() and (ref2["inst"][k == 3] >= 0).all()
        for cull in (0x01, 0x02, 0x10, 0x80, 0x5A, 0x00):
            check(sc, orc, segs[:200], gpu_segments(ctx, segs[:200], cull), cull, what="%s cull %#x" % (name, cull))
    bad = invalid_records(sets["across"])
    ref, _ = check(sc, orc, bad, gpu_segments(ctx, bad), what="invalid records")
    assert (ref["inst"][:N_INVALID] == -1).all()
    h, a, s = gpu_segments(ctx, sets["short"], attributes=False, params=False)
    assert a is None and s is None and h.tobytes() == sgr.brute32(sc, sets["short"])[0].tobytes()
    h, a, s = gpu_segments(ctx, sets["short"], attributes=True, params=False)      # (the side words come from the workspace's parameters)
    check(sc, orc, sets["short"], (h, a, None), what="attributes without parameters")
    every = np.concatenate(list(sets.values()) * 2)[:3000]
    assert len(every) == 3000
    for n in (1, 63, 65, 257, 3000):
        check(sc, orc, every[:n], gpu_segments(ctx, every[:n]), what="%d records" % n)


@pytest.mark.gpu
def test_point_identity_on_the_device(ctx):
    """P0 == P1: the hits and attributes are closest_point_device's on the same context byte for byte, s = 0"""
    import torch
    verts, idx, ranges, inst = small_scene(seed=55)
    sc, orc = load(ctx, verts, idx, ranges, inst)
    segs = np.concatenate(list(segment_sets(sc, 300, seed=56, closed=np.nonzero(inst["mesh"] == 0)[0]).values()))
    segs[:, 4:7] = segs[:, 0:3]
    segs[::3, 3] = 0.4
    h, a, s = gpu_segments(ctx, segs)
    res = ctx.closest_point_device(torch.from_numpy(np.ascontiguousarray(segs[:, :4])).to("cuda:0"), attributes=True)
    torch.cuda.synchronize()
    hp, ap = res.numpy()
    assert h.tobytes() == hp.tobytes() and a.tobytes() == ap.tobytes() and (s.view(np.uint32) == 0).all()
    assert (h["inst"] >= 0).mean() > 0.5 and (h["inst"] < 0).any()


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
    moved["transform"][:, [3, 7, 11]] += rng.uniform(-0.3, 0.3, (len(inst), 3)).astype(np.float32)
    sc0 = cr.Scene(verts, idx, ranges, inst)
    segs = np.concatenate(list(segment_sets(sc0, 250, seed=73, closed=np.nonzero(inst["mesh"] == 0)[0]).values()) + [feature_segments(sc0, 100, seed=74)])
    segs[::5, 3] = 0.5
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
                for cull in (0xFF, 0x5A):
                    check(sc, orc, segs, gpu_segments(c, segs, cull), cull, "%s records, update %d, builder %s" % (source, update, builder))
        t = deform(geom, 0, amp=0.2)
        torch.cuda.synchronize()
        c.refit_blas_device(0, t)
        torch.cuda.synchronize()
        c.set_instances_device(dev_inst(inst))
        v2 = with_mesh(geom, verts, 0, t)
        check(cr.Scene(v2, idx, ranges, inst), oracle_scene(v2, idx, ranges, inst), segs, gpu_segments(c, segs), what="refit, builder %s" % builder)
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
    sets = segment_sets(sc, 400, seed=82, closed=np.nonzero(inst["mesh"] == 0)[0])
    sets["features"] = feature_segments(sc, 150, seed=84)
    for sname, segs in sets.items():
        ref, _ = check(sc, orc, segs, gpu_segments(ctx, segs), what="%s %s" % (name, sname))
        q = segs.copy(); q[:, 3] = ref["t"] * np.float32(1.25)
        check(sc, orc, q, gpu_segments(ctx, q), what="%s %s radii" % (name, sname))


@pytest.mark.gpu
def test_degenerate_triangles_and_a_singular_instance(ctx):
    """needles and zero-area triangles, and a singular (flattened) instance among them: byte-equal, no NaN t"""
    verts, idx, ranges = degenerate_soup(62)
    inst = placed_instances(12, 63, spacing=2.5, n_meshes=1)
    M = np.asarray(inst[3]["transform"], np.float64).reshape(3, 4)
    M[:, 2] = 0.0                                   # a flattened body: o2w is singular, its boxes do not prune
    inst[3]["transform"] = M.astype(np.float32).reshape(12)
    with np.errstate(all="ignore"):                 # (the reference's inverse of the singular record is not finite, as the library's)
        sc, orc = load(ctx, verts, idx, ranges, inst)
    sets = segment_sets(sc, 400, seed=64, closed=np.arange(len(inst)))
    sets["features"] = feature_segments(sc, 150, seed=65)
    for name, segs in sets.items():
        h, a, s = gpu_segments(ctx, segs, attributes=False)
        assert not np.isnan(h["t"]).any() and not np.isnan(s).any()
        check(sc, orc, segs, (h, None, s), what="degenerate " + name)
        check(sc, orc, segs[:150], gpu_segments(ctx, segs[:150]), what="degenerate %s with attributes" % name)
        q = segs.copy(); q[:, 3] = 0.3
        check(sc, orc, q, gpu_segments(ctx, q, attributes=False), what="degenerate %s radius" % name)


class SegmentQuery:
    """tests/stack_reference.py's model of this walk's descent: rule BOUND on test (i) of csrc/kernels_segment.inc, the squared per-axis
    gap between the segment's interval and the child's box times the instance's scale squared, the smaller bound first; a child is
    entered while its bound does not exceed the search radius squared.  (Test (ii) only ever closes more boxes once a radius is
    finite: the model's `first` peaks are asserted for r_max = inf, its `full` peaks are upper bounds.)"""
    rule = "bound"

    def __init__(self, p0, p1, radius=np.inf, scale2=1.0):
        self.p0, self.p1, self.radius, self.scale2 = [float(x) for x in p0], [float(x) for x in p1], float(radius), float(scale2)

    def into(self, M, scale):
        f = lambda p: [M[a][0] * p[0] + M[a][1] * p[1] + M[a][2] * p[2] + M[a][3] for a in range(3)]   # noqa: E731
        return SegmentQuery(f(self.p0), f(self.p1), self.radius, scale * scale)

    def test(self, lo, hi):
        d2 = 0.0
        for a in range(3):
            d = max(lo[a] - max(self.p0[a], self.p1[a]), min(self.p0[a], self.p1[a]) - hi[a], 0.0)
            d2 += d * d
        d2 *= self.scale2
        return not (d2 > self.radius * self.radius), d2


@pytest.mark.gpu
def test_the_spill_half_of_the_stack():
    """the corridor scene of tests/test_stack_spill.py: segments off the ends of the deep corridors reach STACK2_LDS + 2 entries before
    the first triangle is tested, those at the ladder's foot stay in LDS, interleaved in one call; byte for byte"""
    from tests import test_stack_spill as tss
    small = tss.World(placed=tss.PLACED_SMALL)
    try:
        rays, tag, _ = tss.corridor_rays(tss.SMALL_TARGETS, 4, seed=16, placed=tss.PLACED_SMALL, inside=0.0)
        p0 = rays[:, 0:3] + np.float32(2.0) * rays[:, 4:7]                      # 3 off an end of the row, inside the footprint
        rng = np.random.default_rng(17)
        p1 = p0 + np.float32(1.5) * rays[:, 4:7] + rng.uniform(-0.5, 0.5, (len(p0), 3)).astype(np.float32)
        r = np.where(np.arange(len(p0)) % 7 == 6, 4.0, np.inf)
        r[tag == -1] = 5.0
        r[tag == 0] = 6.0    # (the shallow end: a radius bounds the walk, so that the model's unpruned walk bounds it too)
        segs = records(p0, p1, r)
        q = [SegmentQuery(x[0:3], x[4:7], x[3]) for x in segs.astype(np.float64)]
        tss.premise(small.model, q, np.where(np.isinf(segs[:, 3]) | (tag == 0), tag, -2), (tss.S_TOP, tss.S_ROT0, tss.S_ROT1, tss.S_SHEAR), sample=3,
                    what="segments")
        h, a, s = gpu_segments(small.ctx, segs)
        ref, s_ref = sgr.brute32(small.sc, segs)
        assert h.tobytes() == ref.tobytes(), np.nonzero(h != ref)[0][:5]
        assert s.tobytes() == s_ref.tobytes()
        assert (ref["inst"][tag == -1] == -1).all() and (ref["inst"][tag >= 0] == tag[tag >= 0]).all()
        kinds, _ = sgr.side_words(small.sc, segs, ref, s_ref)
        assert np.array_equal(a[:, 7].view(np.uint32), kinds)
    finally:
        small.ctx.close()


@pytest.mark.gpu
def test_against_the_sphere_sweep(ctx):
    """500 segments with t > 0: the sphere of radius 1.01 t swept from P0 along P1 - P0 over [0, 1] reports a contact, the sphere of
    radius 0.99 t none.  "t > 0" is t above 1e-3 of the scene's diagonal: a pierced triangle reports a residue above 0 while a sphere of
    any radius touches it, and the sweep's own quadratics lose about 2^-24 (E + r)^2 / r of a radius (include/rt_api.h), which stays
    below a quarter of the 1 % asked here only for r above 0.005 E (E, the triangles' edges, is at most 2.8 on this scene of diagonal 18.7)"""
    import torch
    verts, idx, ranges, inst = small_scene(seed=91)
    sc, orc = load(ctx, verts, idx, ranges, inst)
    sets = segment_sets(sc, 400, seed=92, closed=np.nonzero(inst["mesh"] == 0)[0])
    segs = np.concatenate([sets["short"], sets["inside"], sets["axis"], sets["edge-parallel"]])
    h, _, _ = gpu_segments(ctx, segs, attributes=False)
    lo, hi = scene_box(sc)
    keep = np.nonzero(h["t"] > 1e-3 * np.linalg.norm(hi - lo))[0][:500]      # (clear of the residues of pierced triangles)
    assert len(keep) == 500
    segs, t = segs[keep], h["t"][keep]
    for factor, contact in ((1.01, True), (0.99, False)):
        sw = np.zeros((len(segs), 8), np.float32)
        sw[:, 0:3] = segs[:, 0:3]; sw[:, 3] = t * np.float32(factor); sw[:, 4:7] = segs[:, 4:7] - segs[:, 0:3]; sw[:, 7] = 1.0
        res = ctx.sweep_spheres_device(torch.from_numpy(sw).to("cuda:0"))
        torch.cuda.synchronize()
        hs = res.numpy()[0]
        assert ((hs["inst"] >= 0) == contact).all(), (factor, np.nonzero((hs["inst"] >= 0) != contact)[0][:5])


@pytest.mark.gpu
def test_plumbing(ctx):
    """host form = device form; counting; out= reuse; stream order behind a slow queue on a side stream; interleaving with
    rt_intersect_device, rt_closest_point_device and rt_shade_rays_device; n == 0"""
    import torch
    from tests.test_ray_query import mixed_rays
    sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
    g = sp.geom
    sc, orc = load(ctx, g.verts, g.idx, g.ranges, sp.instances)
    ctx.set_uniforms(sp.uniforms)
    segs = np.concatenate(list(segment_sets(sc, 100, seed=102, closed=np.arange(len(sp.instances))).values()))
    segs[::4, 3] = 0.5
    ref, s_ref = check(sc, orc, segs, gpu_segments(ctx, segs), what="device form")
    hh, st = ctx.closest_segment(segs)
    assert hh.tobytes() == ref.tobytes() and st.node_visits == 0 and st.bvh_node_bytes > 0
    hc, s_host, st = ctx.closest_segment(segs, params=True, counting=True)
    assert hc.tobytes() == ref.tobytes() and s_host.tobytes() == s_ref.tobytes() and st.node_visits > 0 and st.tri_tests > 0
    assert ctx.closest_segment(segs, cull_mask=0)[0]["inst"].max() == -1
    # out= reuse
    src = dev(segs)
    n = len(segs)
    hits = torch.empty((n, 5), dtype=torch.int32, device="cuda:0"); attr = torch.empty((n, 8), dtype=torch.int32, device="cuda:0")
    par = torch.empty((n,), dtype=torch.float32, device="cuda:0")
    res = ctx.closest_segment_device(src, attributes=True, params=True, out=(hits, attr, par))
    assert res.hits.data_ptr() == hits.data_ptr() and res.attr.data_ptr() == attr.data_ptr() and res.s.data_ptr() == par.data_ptr()
    assert res.numpy()[0].tobytes() == ref.tobytes() and res.s.cpu().numpy().tobytes() == s_ref.tobytes()
    with pytest.raises(ValueError):
        ctx.closest_segment_device(src, out=(hits[:-1], None))
    with pytest.raises(ValueError):
        ctx.closest_segment_device(src, params=True, out=(hits, None, par[:-1]))
    # stream order
    rays = torch.from_numpy(mixed_rays(n, seed=103)).to("cuda:0")
    closest = ctx.intersect_device(rays).numpy()[0]
    pts = src[:, :4].contiguous()
    near = ctx.closest_point_device(pts).numpy()[0]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = slow_queue(torch, 12)
        p = (src + (a[0, 0] != a[0, 0]).to(torch.float32) * 0).contiguous()   # made behind the queue, on the side stream
        r1 = ctx.closest_segment_device(p, attributes=True, params=True, stream=side)
        q1 = ctx.intersect_device(rays, stream=side)
        c1 = ctx.closest_point_device(pts, stream=side)
        img = ctx.shade_rays_device(rays, stream=side)                         # a shading call between two segment queries
        r2 = ctx.closest_segment_device(p, stream=side)
        p.zero_()                                                             # overwritten right after the calls
        h1, h2, hq, hp, s1 = r1.hits.clone(), r2.hits.clone(), q1.hits.clone(), c1.hits.clone(), r1.s.clone()
    side.synchronize()
    assert img is not None and img[1] is not None and tuple(img[1].shape) == (rays.shape[0], 4)
    for hcopy in (h1, h2):
        assert hcopy.cpu().numpy().view(HIT_DTYPE).reshape(-1).tobytes() == ref.tobytes()
    assert s1.cpu().numpy().tobytes() == s_ref.tobytes()
    assert hq.cpu().numpy().view(HIT_DTYPE).reshape(-1).tobytes() == closest.tobytes()
    assert hp.cpu().numpy().view(HIT_DTYPE).reshape(-1).tobytes() == near.tobytes()
    # n == 0
    e = ctx.closest_segment_device(torch.empty((0, 8), dtype=torch.float32, device="cuda:0"), attributes=True, params=True)
    assert e.hits.shape == (0, 5) and e.attr.shape == (0, 8) and e.s.shape == (0,)
    assert len(ctx.closest_segment(np.zeros((0, 8), np.float32))[0]) == 0
    # device tensors through capsule_records
    rec = api.capsule_records(src[:, 0:3], src[:, 4:7], src[:, 3])
    assert rec.is_cuda and torch.equal(rec[:, :7], src[:, :7])


def _raw(c, n, segs, cull, hits, attr, par):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_closest_segment_device(c.h, n, p(segs), cull, p(hits), p(attr), p(par), None)


@pytest.mark.gpu
def test_error_statuses():
    import torch
    verts, idx, ranges, inst = small_scene(seed=121)
    sc = cr.Scene(verts, idx, ranges, inst)
    segs_np = segment_sets(sc, 300, seed=122, closed=np.nonzero(inst["mesh"] == 0)[0])["short"]
    ref, _ = sgr.brute32(sc, segs_np)
    segs = dev(segs_np)
    n = segs.shape[0]
    hits = torch.empty((n + 1, 5), dtype=torch.int32, device="cuda:0")
    attr = torch.empty((n + 1, 8), dtype=torch.int32, device="cuda:0")
    par = torch.empty((n + 1,), dtype=torch.float32, device="cuda:0")
    S_, H_, A_, P_ = segs.data_ptr(), hits.data_ptr(), attr.data_ptr(), par.data_ptr()
    c = RtContext(0)

    def err(args, code, text):
        assert _raw(c, *args) == code, args
        msg = c.L.rt_last_error(c.h).decode()
        assert text in msg, (args, msg)

    def ok():
        assert c.closest_segment_device(segs).numpy()[0].tobytes() == ref.tobytes()

    try:
        err((n, S_, 0xFF, H_, 0, 0), RT_ERR_NOT_READY, "")   # no geometry
        c.upload_geometry(verts, idx, ranges)
        err((n, S_, 0xFF, H_, 0, 0), RT_ERR_NOT_READY, "")   # no TLAS
        c.set_instances(inst)
        ok()
        bad = [((0xFFFFFF00, S_, 0xFF, H_, 0, 0), "too many segments"), ((n, S_, 0x100, H_, 0, 0), "cull_mask"), ((n, 0, 0xFF, H_, 0, 0), "null segment/hit pointers"),
               ((n, S_, 0xFF, 0, 0, 0), "null segment/hit pointers"), ((n, S_ + 4, 0xFF, H_, 0, 0), "aligned"), ((n, S_, 0xFF, H_ + 2, 0, 0), "aligned"),
               ((n, S_, 0xFF, H_, A_ + 4, 0), "aligned"), ((n, S_, 0xFF, H_, 0, P_ + 2), "aligned")]
        host_buf = np.zeros((n + 1, 8), np.float32)
        pinned = torch.zeros((n, 8), dtype=torch.float32).pin_memory()
        for ptr in ((host_buf.ctypes.data + 15) & ~15, pinned.data_ptr()):   # (16-byte aligned: only the memory kind is wrong)
            bad += [((n, ptr, 0xFF, H_, 0, 0), "device memory of the context's GPU"), ((n, S_, 0xFF, ptr, 0, 0), "device memory of the context's GPU"),
                    ((n, S_, 0xFF, H_, ptr, 0), "device memory of the context's GPU"), ((n, S_, 0xFF, H_, 0, ptr), "device memory of the context's GPU")]
        for args, text in bad:
            err(args, RT_ERR_INVALID_ARGUMENT, text)
            ok()
        out = np.zeros(n, HIT_DTYPE)
        assert c.L.rt_closest_segment(c.h, n, None, 0xFF, out.ctypes.data_as(ctypes.c_void_p), None, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_closest_segment(c.h, n, segs_np.ctypes.data_as(ctypes.c_void_p), 0x100, out.ctypes.data_as(ctypes.c_void_p), None, 0, None) == RT_ERR_INVALID_ARGUMENT
        ok()
        assert _raw(c, 0, 0, 0xFF, 0, 0, 0) == 0   # n == 0 enqueues nothing and needs no pointers
        with pytest.raises(ValueError):
            c.closest_segment_device(segs.cpu())
        with pytest.raises(ValueError):
            c.closest_segment_device(torch.zeros((4, 4), dtype=torch.float32, device="cuda:0"))
        with pytest.raises(RtError) as e:
            c.closest_segment_device(segs, cull_mask=0x1FF)
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
