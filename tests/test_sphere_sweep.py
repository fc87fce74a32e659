"""rt_sweep_spheres_device / rt_sweep_spheres: the first contact of a sphere that moves along a direction.

tests/sweep_reference.py holds the two references: brute32, the canonical binary32 contact time of include/rt_api.h and DESIGN.md §5
"Sphere sweeps" restated in numpy over (sweep, instance, triangle), and brute64, the exact first-contact time in binary64 on the same
binary32 inputs.  The CPU part holds brute32 to brute64 by a sandwich in the radius (contact time is non-increasing in the radius); the
GPU part holds the library to brute32 byte for byte: under every tree the library can build, far from the origin, under sheared, scaled
and singular instances, on degenerate geometry, with attributes, and the plumbing of a device query."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import closest_reference as cr
from tests import scenes
from tests import sweep_reference as sr
from tests.test_closest_point import scene_box, small_scene, surface_points, teapot_scene
from tests.test_overlap_boxes import SCENES, cancelling_scene, lattice_scene
from tests.test_ray_query import PATHS, dev_inst, slow_queue
from tests.test_ray_query_oracle import oracle_scene, placed_instances, small_meshes, use_builder
from vulkan_raytracing_amd import RtContext, api
from vulkan_raytracing_amd.api import HIT_DTYPE, RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
INF = np.float32(np.inf)
EPS = 2.0 ** -24
# The constant of the binary64 sandwich.  Measured over powers of two, the smallest for which brute32 holds on every committed set is 4
# (small `grazing` and small+10000 `misc`; 1 or 2 on every other scene and set); the test uses the power of two at 4 times that
# (DESIGN.md §5 "Sphere sweeps").
K_MEASURED, K = 4, 16


# ---- scenes and sweep sets ----------------------------------------------------------------------------------------------------

def as_sweeps(o, r, d, tmax):
    n = len(o)
    s = np.zeros((n, 8), np.float64)
    s[:, 0:3] = o; s[:, 3] = r; s[:, 4:7] = d; s[:, 7] = tmax
    return s.astype(np.float32)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def invalid_sweeps(s):
    """records the contract answers with the miss form: a non-finite component of o, d or r, r < 0, d = 0, tmax < 0, a NaN tmax; then
    four valid edge values (r = -0, tmax = -0, tmax = 0, a huge finite tmax)"""
    q = np.array(s[:16], np.float32).copy()
    q[0, 0] = np.nan; q[1, 1] = np.inf; q[2, 2] = -np.inf; q[3, 3] = np.nan; q[4, 3] = np.inf; q[5, 3] = -1e-3
    q[6, 4] = np.nan; q[7, 5] = np.inf; q[8, 6] = -np.inf; q[9, 4:7] = 0.0; q[10, 7] = -1.0; q[11, 7] = np.nan
    q[12, 3] = np.float32(-0.0); q[13, 7] = np.float32(-0.0); q[14, 7] = 0.0; q[15, 7] = 3e38
    return q


N_INVALID = 12


def sweep_sets(sc, n, seed):
    """five sets of about n records (see the issue's names): `aimed` from outside the scene box towards surface points, radii log-uniform
    from 1e-3 to 0.2 of the scene extent; `grazing` paths that pass edges and vertices at r (1 +- 1e-3); `inside` origins within r of
    the surface; `long` origins 3 to 50 extents out; `misc` r = 0, tmax short of the contact, tmax = inf, unnormalised d of length 1e-3
    to 1e3, and every invalid record"""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(sc)
    c, ext = (lo + hi) / 2, (hi - lo).max()
    diag = np.linalg.norm(hi - lo)

    def radii(m):
        return ext * 10 ** rng.uniform(-3, np.log10(0.2), m)

    def outside(m, lo_f, hi_f):
        return c + unit(rng.normal(size=(m, 3))) * diag * rng.uniform(lo_f, hi_f, (m, 1))

    tgt = surface_points(sc, n, rng, 0.0)
    o = outside(n, 0.8, 1.5)
    aimed = as_sweeps(o, radii(n), unit(tgt - o), np.inf)
    # grazing: a point P of an edge (a vertex for every third record), a direction d, a unit w perpendicular to d (and to the edge):
    # the path passes P at the distance r (1 +- 1e-3) along w
    k = rng.integers(0, sc.n_tris, n)
    e = sc.B[k] - sc.A[k]
    s = np.where((np.arange(n) % 3 == 0)[:, None], rng.integers(0, 2, (n, 1)).astype(np.float64), rng.uniform(size=(n, 1)))
    P = sc.A[k] + s * e
    d = unit(rng.normal(size=(n, 3)))
    w = np.cross(d, np.where(np.linalg.norm(e, axis=1, keepdims=True) > 0, e, rng.normal(size=(n, 3))))
    w = unit(np.where(np.linalg.norm(w, axis=1, keepdims=True) > 1e-9, w, np.cross(d, rng.normal(size=(n, 3)))))
    r = radii(n)
    off = r * (1 + 1e-3 * rng.choice([-1.0, 1.0], n))
    grazing = as_sweeps(P + w * off[:, None] - d * diag * rng.uniform(0.5, 1.5, (n, 1)), r, d, np.inf)
    r = radii(n)
    p = surface_points(sc, n, rng, 0.0) + unit(rng.normal(size=(n, 3))) * (r * rng.uniform(0, 1, n))[:, None]
    inside = as_sweeps(p, r, unit(rng.normal(size=(n, 3))), diag * rng.uniform(0.1, 2.0, n))
    tgt = surface_points(sc, n, rng, 0.0)
    o = c + unit(rng.normal(size=(n, 3))) * ext * rng.uniform(3, 50, (n, 1))
    long_ = as_sweeps(o, radii(n), unit(tgt - o), np.inf)
    m = n // 4
    tgt = surface_points(sc, 4 * m, rng, 0.0)
    o = outside(4 * m, 0.8, 1.5)
    dist = np.linalg.norm(tgt - o, axis=1)
    r = radii(4 * m)
    ln = 10 ** rng.uniform(-3, 3, m)
    misc = np.concatenate([
        as_sweeps(o[:m], 0.0, unit(tgt[:m] - o[:m]), np.inf),
        as_sweeps(o[m:2 * m], r[m:2 * m], unit(tgt[m:2 * m] - o[m:2 * m]), dist[m:2 * m] * rng.uniform(0.2, 1.1, m)),
        as_sweeps(o[2 * m:3 * m], r[2 * m:3 * m], unit(tgt[2 * m:3 * m] - o[2 * m:3 * m]) * ln[:, None],
                  np.where(np.arange(m) % 2 == 0, np.inf, 2 * dist[2 * m:3 * m] / ln)),
        as_sweeps(o[3 * m:], r[3 * m:], unit(rng.normal(size=(m, 3))), np.inf)])   # (unaimed: many miss)
    misc = np.concatenate([misc, invalid_sweeps(misc[2 * m:])])
    return {"aimed": aimed, "grazing": grazing, "inside": inside, "long": long_, "misc": misc}


def lattice_sweeps(sc):
    """integer radii and axis-parallel unit directions around lattice_scene: from integer origins on a grid (mostly vertex and edge
    contacts), and onto interior points with dyadic barycentrics of the triangles whose normal is parallel to an axis, along that axis
    (face contacts in which every operation is exact; a face whose normal has an irrational length has no exact contact time)"""
    x, y = np.meshgrid(np.arange(-10, 8), np.arange(-8, 8), indexing="ij")
    g = np.stack([x.reshape(-1), y.reshape(-1)], axis=1).astype(np.float64)
    out = []
    for r in (1.0, 2.0):
        for axis in range(3):
            for sign in (1.0, -1.0):
                o = np.zeros((len(g), 3)); d = np.zeros((len(g), 3))
                o[:, (axis + 1) % 3] = g[:, 0]; o[:, (axis + 2) % 3] = g[:, 1]
                o[:, axis] = -32.0 * sign; d[:, axis] = sign
                out.append(as_sweeps(o, r, d, np.inf))
    grid = np.concatenate(out)[::2]
    N = np.cross(sc.B - sc.A, sc.C - sc.A)
    flat = np.nonzero((N != 0).sum(axis=1) == 1)[0]
    out = []
    for k in flat:
        axis = int(np.nonzero(N[k])[0][0])
        for bu, bv in ((0.25, 0.25), (0.5, 0.25), (0.25, 0.5), (0.125, 0.125), (0.75, 0.125), (0.125, 0.75), (0.375, 0.375), (0.5, 0.375)):
            tgt = sc.A[k] + bu * (sc.B[k] - sc.A[k]) + bv * (sc.C[k] - sc.A[k])
            for sign in (1.0, -1.0):
                for r in (1.0, 2.0, 3.0):
                    d = np.zeros(3); d[axis] = sign
                    out.append(as_sweeps((tgt - 32.0 * d)[None], r, d[None], np.inf))
    return np.concatenate([grid] + out)


def sheared_scene(seed=211):
    """small_meshes under strongly sheared and non-uniformly scaled instances (axis scales 0.2 to 5), and one singular instance (a
    flattened mesh: s_i = 0, its boxes do not prune)"""
    verts, idx, ranges = small_meshes(seed)
    inst = placed_instances(12, seed + 1, spacing=4.0)
    rng = np.random.default_rng(seed + 2)
    for i in range(len(inst)):
        M = np.asarray(inst[i]["transform"], np.float64).reshape(3, 4)
        S = np.diag(10 ** rng.uniform(-0.7, 0.7, 3))
        S[0, 1] = rng.uniform(-1.5, 1.5); S[1, 2] = rng.uniform(-1.5, 1.5)
        if i == 5:
            S[2, :] = 0.0   # singular
        M[:, :3] = M[:, :3] @ S
        inst[i]["transform"] = M.astype(np.float32).reshape(12)
    return verts, idx, ranges, inst


ALL_SCENES = dict(SCENES)
ALL_SCENES.update({"lattice": lattice_scene, "cancel": cancelling_scene, "sheared": sheared_scene})
_CACHE = {}


def scene_and_sets(name):
    """the scene, its sweep sets and brute32 of every set (with the candidate pairs it ran over), computed once"""
    if name not in _CACHE:
        parts = small_scene(seed=161, offset=float(name[6:])) if name.startswith("small+") else ALL_SCENES[name]()
        sc = cr.Scene(*parts)
        sets = {"lattice": lattice_sweeps(sc)} if name == "lattice" else sweep_sets(sc, 120 if name == "teapot" else 2000, seed=202)
        # (the teapot, 13 536 small triangles: about 800 candidate pairs per record against 30 on the other scenes, whose numpy
        # restatement costs 18 s per 400 records and set; its 616 records keep the CPU test at 5 s.  DESIGN.md §5 says so.)
        pairs = {k: sr.candidate_pairs(sc, s) for k, s in sets.items()}
        ref = {k: sr.brute32(sc, s, pairs=pairs[k]) for k, s in sets.items()}
        _CACHE[name] = (parts, sc, sets, pairs, ref)
    return _CACHE[name]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_exports_abi_and_null_context():
    assert "rt_sweep_spheres_device" in api.EXPORTS and "rt_sweep_spheres" in api.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^int rt_sweep_spheres_device\(rt_ctx\* ctx, size_t n, const void\* d_sweeps8, uint32_t cull_mask,\s+void\* d_hits, void\* d_attr, "
                     r"void\* hip_stream\);", hdr, re.M)
    assert re.search(r"^int rt_sweep_spheres\(rt_ctx\* ctx, size_t n, const float\* sweeps8_host, uint32_t cull_mask,\s+rt_hit\* out_host, int counting, "
                     r"rt_stats\* stats\);", hdr, re.M)
    L = api.lib()
    assert hasattr(L, "rt_sweep_spheres_device") and hasattr(L, "rt_sweep_spheres") and L.rt_abi_version() == 7
    assert L.rt_sweep_spheres_device(None, 0, None, 0xFF, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_sweep_spheres_device(None, 64, None, 0xFF, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_sweep_spheres(None, 0, None, 0xFF, None, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert hasattr(RtContext, "sweep_spheres_device") and hasattr(RtContext, "sweep_spheres")


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_sweep_kernels_use_no_scratch(target):
    """exactly two new walk kernels, k_sweep_spheres and its counting form, and k_sweep_side, in both libraries: no scratch, no spills, and
    the walks within the record-level budget (>= 4 waves per SIMD)"""
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    walk = [(n, r) for n, r in kernels.items() if "k_sweep_spheres" in n]
    side = [(n, r) for n, r in kernels.items() if "k_sweep_side" in n]
    assert len(walk) == 2 and len(side) == 1 and sum("k_sweep_spheres_count" in n for n, _ in walk) == 1, "\n".join(kernels)
    for name, r in walk + side:
        assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
    for name, r in walk:
        assert int(r["Occupancy"]) >= 4, (name, r)


def longest_edge(sc, tri):
    e = np.stack([np.linalg.norm(sc.B[tri] - sc.A[tri], axis=1), np.linalg.norm(sc.C[tri] - sc.B[tri], axis=1), np.linalg.norm(sc.A[tri] - sc.C[tri], axis=1)])
    return e.max(axis=0)


def magnitude(sc):
    """the largest magnitude that enters a candidate's world vertices: the world coordinates and the terms of the rows of
    A = xform_point(o2w, v0) (|o2w_r| . |v| + |o2w_r3|), which exceed them when a translation cancels the mesh's own offset"""
    lo, hi = scene_box(sc)
    ov = np.maximum(np.maximum(np.abs(sc.v0), np.abs(sc.v0 + sc.e1)), np.abs(sc.v0 + sc.e2)).astype(np.float64)
    m = np.abs(sc.o2w.astype(np.float64)).reshape(-1, 3, 4)[sc.inst]
    rows = np.einsum("trk,tk->tr", m[:, :, :3], ov) + m[:, :, 3]
    return max(np.abs(lo).max(), np.abs(hi).max(), rows.max())


def sandwich(sc, s, pairs, h, k):
    """per record, the sides of  t64(r + delta) - tau <= t32 <= t64(r - delta) + tau  with the constant k, a miss counting as tmax on
    every side: dict of ok (valid records), lower, t32, upper, delta, tri (the reported triangle's index), t_big (t64(r + delta)) and
    tau_of (t -> tau).  delta = k 2^-24 (M + E^2 / max(r, tiny)): M the largest magnitude of the scene (magnitude()) and of the origin,
    E the longest edge of the reported triangle (of the binary64 triangle for a miss, 0 without either), tiny = 2^-12 E: below it the
    squared radius is lost in 2^-24 E^2 and the loss of the quadratics is sqrt(2^-24) E, not 2^-24 E^2 / r.
    tau = delta / |d| + k 2^-24 t.  Where r < delta there is no smaller sphere to compare with and the upper side asks nothing
    (test_restatement_edge_cases holds r = 0 to the ray reference instead)."""
    s64 = s.astype(np.float64)
    ok = sr.valid_sweeps(s)
    r, tmax = s64[:, 3], s64[:, 7]
    first = np.concatenate([[0], np.cumsum(np.bincount(sc.inst, minlength=len(sc.mask)))])
    hit = h["inst"] >= 0
    t64, tri64 = sr.brute64(sc, s, pairs=pairs)
    tri = np.where(hit, first[np.clip(h["inst"], 0, None)] + h["prim"], tri64)
    E = np.where(tri >= 0, longest_edge(sc, np.clip(tri, 0, None)), 0.0)
    with np.errstate(all="ignore"):
        M = np.maximum(np.abs(np.where(ok[:, None], s64[:, 0:3], 0.0)).max(axis=1), magnitude(sc))
        delta = np.where(ok, k * EPS * (M + E * E / np.maximum(np.maximum(r, 2.0 ** -12 * E), 1e-300)), 0.0)
        dn = np.linalg.norm(s64[:, 4:7], axis=1)
        wide = sr.candidate_pairs(sc, s, extra=float(delta.max(initial=0.0)))
        t_big, _ = sr.brute64(sc, s, radius=r + delta, pairs=wide)
        t_small, _ = sr.brute64(sc, s, radius=np.maximum(r - delta, 0.0), pairs=wide)
        t_small = np.where(r - delta < 0, np.inf, t_small)
        t32 = np.where(hit, h["t"].astype(np.float64), tmax)
        tau_of = lambda t: delta / dn + k * EPS * np.where(np.isfinite(t), t, 0.0)   # noqa: E731
        lower = np.minimum(t_big, tmax); upper = np.minimum(t_small, tmax)
        lower, upper = lower - tau_of(lower), upper + tau_of(upper)
    return dict(ok=ok, lower=lower, t32=t32, upper=upper, delta=delta, tri=tri, t_big=t_big, tau_of=tau_of, two_sided=ok & (r >= delta))


@pytest.mark.parametrize("name", ["small", "teapot", "small+1000", "small+10000", "cancel", "lattice"])
def test_binary32_restatement_against_binary64(name):
    """the sandwich t64(r + delta) - tau <= t32 <= t64(r - delta) + tau on every record of every set, none excused; the binary64 distance
    from p(t32) to the reported triangle is within delta of r (at most r + delta where t32 = 0); the upper side is active (r >= delta) on
    at least three quarters of the valid records with r > 0 of every set, and the share is printed; on the lattice t32 == t64 for the face
    contacts whose arithmetic is exact (a normal parallel to an axis: the length of any other normal is irrational).
    soup and sliver do not join: their needles (aspect 1e-4) and zero-area triangles make the face's 2 x 2 system and the edge
    quadratics rounding noise; the GPU tests cover them bit for bit."""
    parts, sc, sets, pairs, ref = scene_and_sets(name)
    for k_set, s in sets.items():
        h = ref[k_set]
        w = sandwich(sc, s, pairs[k_set], h, K)
        ok, lower, t32, upper, delta, tri = (w[x] for x in ("ok", "lower", "t32", "upper", "delta", "tri"))
        hit = h["inst"] >= 0
        assert not hit[~ok].any()
        with np.errstate(invalid="ignore"):
            good = ~ok | ((lower <= t32) & (t32 <= upper))
        sized = ok & (s[:, 3] > 0)
        share = w["two_sided"][sized].mean()
        print("%s %s: %d records, %d hits, %d outside the sandwich, upper side active on %.3f of the valid records with r > 0" %
              (name, k_set, len(s), hit.sum(), (~good).sum(), share))
        # (the sandwich must stay two-sided: radii are log-uniform over 2.3 decades from 1e-3 of the extent, and delta reaches the lowest
        # quarter of that range, 3.7e-3 of the extent, only where M exceeds 200 extents; no committed scene is there)
        assert share >= 0.75, (k_set, share)
        assert good.all(), (k_set, np.nonzero(~good)[0][:5], lower[~good][:5], t32[~good][:5], upper[~good][:5])
        s64 = s.astype(np.float64)
        p = s64[hit, 0:3] + t32[hit, None] * s64[hit, 4:7]
        dist = sr.distance64(sc, p, tri[hit])
        r = s64[hit, 3]
        touching = np.where(t32[hit] == 0, dist <= r + delta[hit], np.abs(dist - r) <= delta[hit])
        assert touching.all(), (k_set, np.abs(dist - r)[~touching][:5], delta[hit][~touching][:5])
        if name == "lattice":
            # face contacts on triangles whose normal is parallel to an axis: every operation is exact in binary32 and binary64 alike
            t64, tri64 = sr.brute64(sc, s, pairs=pairs[k_set])
            N = np.cross(sc.B - sc.A, sc.C - sc.A)
            exact = hit & (h["u"] > 0) & (h["v"] > 0) & (h["u"] + h["v"] < 1) & ((N != 0).sum(axis=1) == 1)[np.clip(tri, 0, None)]
            assert exact.sum() >= 64 and np.array_equal(t32[exact], t64[exact])


def test_restatement_edge_cases():
    """every invalid record gives the miss form; t = 0 inside; the tmax cut-off (misses: where nothing was hit tmax = inf * 0.5 = inf); the tie order between two coplanar instances; r = 0
    against query_reference's ray hit within the sandwich's bound, away from edges"""
    from tests import query_reference as qr
    parts, sc, sets, pairs, ref = scene_and_sets("small")
    misc, h = sets["misc"], ref["misc"]
    bad = ~sr.valid_sweeps(misc)
    assert bad.sum() == N_INVALID and (h["inst"][bad] == -1).all() and (h["prim"][bad] == -1).all() and (h["u"][bad] == 0).all() and (h["v"][bad] == 0).all()
    assert np.array_equal(h["t"][bad].view(np.uint32), misc[bad, 7].view(np.uint32))
    assert not np.isnan(h["t"][~np.isnan(misc[:, 7])]).any()
    # t = 0 inside: origins on the surface itself
    rng = np.random.default_rng(203)
    p = surface_points(sc, 300, rng, 0.0)
    on = as_sweeps(p, 0.05, unit(rng.normal(size=(300, 3))), 1.0)
    z = sr.brute32(sc, on)
    near = cr.brute32(sc, np.concatenate([on[:, 0:3], np.full((300, 1), 0.05, np.float32)], axis=1))
    # (some instances of the scene have a mask the call does not admit: a point on their surface may be far from every other one)
    assert np.array_equal(z["inst"] >= 0, near["inst"] >= 0) | (z["inst"] >= 0).all()
    got = near["inst"] >= 0
    assert got.mean() > 0.8 and (z["t"][got] == 0).all()
    # (the closest triangle is among those the sphere overlaps; the sweep reports the smallest (inst, prim) of them)
    assert ((z["inst"] < near["inst"]) | ((z["inst"] == near["inst"]) & (z["prim"] <= near["prim"])))[got].all()
    # tmax cut-off: just beyond the contact it is found, short of it the record misses with tmax as given
    a, ha = sets["aimed"][:500], ref["aimed"][:500]
    got = ha["inst"] >= 0
    assert got.mean() > 0.9
    # (t_c is clamped to tmax, so a shorter tmax may round the same contact differently: t moves by rounding, and with it the choice
    # among triangles that share the touched edge or vertex)
    q = a.copy(); q[:, 7] = np.where(got, ha["t"] * np.float32(1.01), 1.0)
    beyond = sr.brute32(sc, q)
    assert (beyond["inst"][got] == ha["inst"][got]).all() and (beyond["prim"][got] == ha["prim"][got]).mean() > 0.9 and (beyond["t"] <= q[:, 7]).all()
    assert np.allclose(beyond["t"][got], ha["t"][got], rtol=1e-5, atol=0)
    q[:, 7] = ha["t"] * np.float32(0.5)
    cut = sr.brute32(sc, q)
    assert (cut["inst"][got] == -1).all() and np.array_equal(cut["t"][got], q[got, 7]) and (cut["u"][got] == 0).all()
    # tie order: the same mesh twice at the same place: the smaller instance index is reported, whichever comes first in the records
    verts, idx, ranges, inst = parts
    two = np.concatenate([inst[3:4], inst[:3], inst[3:4]])
    two["custom_index_and_mask"] |= np.uint32(0xFF << 24)
    sc2 = cr.Scene(verts, idx, ranges, two)
    s2 = sweep_sets(cr.Scene(verts, idx, ranges, inst[3:4]), 200, seed=204)["aimed"]
    h2 = sr.brute32(sc2, s2)
    one = sr.brute32(cr.Scene(verts, idx, ranges, two[:4]), s2)
    assert h2.tobytes() == one.tobytes() and (h2["inst"] == 0).sum() > 100 and not (h2["inst"] == 4).any()
    # r = 0 against the ray reference, away from edges: the same triangle; there the contact time is linear in the radius, so the ray's
    # t is at most t(0) - t(delta) later than the lower side allows, and t32 lies within that of the ray's t
    m = len(misc) // 4 - 4
    rays = misc[:m].copy()
    assert (rays[:, 3] == 0).all() and np.isinf(rays[:, 7]).all()   # (r = 0 where a ray has tmin = 0)
    rays[:, 7] = 1e6                                                 # (the ray reference wants a finite tmax)
    want = qr.query(qr.Scene(*parts), rays)
    w = sandwich(sc, misc[:m], sr.candidate_pairs(sc, misc[:m]), h[:m], K)
    inner = (want["inst"] >= 0) & ~want["ambiguous"] & (want["u"] > 0.02) & (want["v"] > 0.02) & (want["u"] + want["v"] < 0.98)
    assert inner.sum() > 100
    assert (want["inst"][inner] == h["inst"][:m][inner]).all() and (want["prim"][inner] == h["prim"][:m][inner]).all()
    slack = (want["t"] - w["t_big"]) + w["tau_of"](want["t"])
    assert (slack[inner] >= 0).all() and (np.abs(w["t32"] - want["t"]) <= slack)[inner].all()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


def dev(s):
    import torch
    return torch.from_numpy(np.ascontiguousarray(s, np.float32).reshape(-1, 8)).to("cuda:0")


def gpu_sweep(c, s, cull=0xFF, attributes=False):
    import torch
    res = c.sweep_spheres_device(dev(s), cull_mask=cull, attributes=attributes)
    torch.cuda.synchronize()
    return res.numpy()


def check(h, ref, s, what):
    """the GPU's hit records against brute32's byte for byte; t is never NaN unless tmax was"""
    if h.tobytes() != ref.tobytes():
        bad = np.nonzero((h.view(np.uint8).reshape(len(h), -1) != ref.view(np.uint8).reshape(len(h), -1)).any(axis=1))[0]
        raise AssertionError("%s: %d of %d records differ from the brute force, first %d: sweep %s gpu %s reference %s" %
                             (what, len(bad), len(h), bad[0], np.asarray(s).reshape(-1, 8)[bad[0]], h[bad[0]], ref[bad[0]]))
    assert not np.isnan(h["t"][~np.isnan(np.asarray(s, np.float32).reshape(-1, 8)[:, 7])]).any(), what


def load(c, parts):
    verts, idx, ranges, inst = parts
    c.upload_geometry(verts, idx, ranges)
    c.set_instances(inst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "teapot", "soup", "sliver"])
def test_every_sweep_set(ctx, name):
    """aimed, grazing, inside, long and misc (r = 0, short and infinite tmax, unnormalised d, invalid records); cull masks"""
    parts, sc, sets, pairs, ref = scene_and_sets(name)
    load(ctx, parts)
    for k, s in sets.items():
        check(gpu_sweep(ctx, s)[0], ref[k], s, "%s %s" % (name, k))
        assert (ref[k]["inst"] >= 0).mean() > 0.3, k
    bad = ~sr.valid_sweeps(sets["misc"])
    assert bad.sum() == N_INVALID and (ref["misc"]["inst"][bad] == -1).all()
    mixed = np.concatenate([s[:400] for s in sets.values()])
    for cull in (0x01, 0x5A, 0x00):
        r = sr.brute32(sc, mixed, cull)
        check(gpu_sweep(ctx, mixed, cull)[0], r, mixed, "%s cull %#x" % (name, cull))
        assert (sc.mask[r["inst"][r["inst"] >= 0]] & cull != 0).all() and (cull != 0 or (r["inst"] == -1).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small+1000", "small+10000", "cancel", "lattice"])
def test_translated_cancelling_and_lattice_scenes(ctx, name):
    """the scene 1 000 and 10 000 units from the origin, instances whose translation cancels their mesh's own offset (the walk's slack
    must cover the rounding of the world vertices), and the integer lattice with its exact ties"""
    parts, sc, sets, pairs, ref = scene_and_sets(name)
    load(ctx, parts)
    for k, s in sets.items():
        check(gpu_sweep(ctx, s)[0], ref[k], s, "%s %s" % (name, k))
        assert (ref[k]["inst"] >= 0).mean() > 0.3, k


@pytest.mark.gpu
def test_sheared_scaled_and_singular_instances(ctx):
    """strong shear and non-uniform scale (the sphere stays a sphere: the sweep runs in world space, the boxes are inflated by r / s_i)
    and one singular instance (s_i = 0: its boxes do not prune, its collinear world triangles are answered by the same arithmetic)"""
    parts, sc, sets, pairs, ref = scene_and_sets("sheared")
    load(ctx, parts)
    L = sc.o2w.reshape(-1, 3, 4)[:, :, :3].astype(np.float64)
    sv = np.linalg.svd(L, compute_uv=False)
    assert (sv[:, 2] < 1e-6).sum() == 1 and (sv[:, 0] / np.maximum(sv[:, 2], 1e-30) > 5).sum() >= 6
    for k, s in sets.items():
        check(gpu_sweep(ctx, s)[0], ref[k], s, "sheared %s" % k)
        assert (ref[k]["inst"] >= 0).mean() > 0.3, k


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "unset", "1", "2"])
def test_tree_independence(builder, monkeypatch):
    """the same sweeps over blas_builder 0 and RT_GPU_BVH_ALGO unset / 1 / 2, host and device instance records with their refits: every
    output equals one brute force, so they are byte-identical to each other"""
    import torch
    parts, sc0, sets, pairs, ref = scene_and_sets("small")
    verts, idx, ranges, inst = parts
    rng = np.random.default_rng(72)
    moved = inst.copy()
    moved["transform"][:, [3, 7, 11]] += rng.uniform(-0.3, 0.3, (len(inst), 3)).astype(np.float32)
    s = np.concatenate([x[:500] for x in sets.values()] + [sets["misc"][-16:]])
    r0 = np.concatenate([ref[k][:500] for k in sets] + [ref["misc"][-16:]])
    r1 = sr.brute32(cr.Scene(verts, idx, ranges, moved), s)
    c = RtContext(0)
    try:
        if builder == "unset":
            monkeypatch.delenv("RT_GPU_BVH_ALGO", raising=False)
            c.set_param("blas_builder", 1)
        else:
            use_builder(c, builder, monkeypatch)
        c.upload_geometry(verts, idx, ranges)
        for source in ("host", "device"):
            for records, update, r in ((inst, False, r0), (moved, True, r1)):
                if source == "host":
                    c.set_instances(records, update=update)
                else:
                    torch.cuda.synchronize()
                    c.set_instances_device(dev_inst(records), update=update)
                check(gpu_sweep(c, s)[0], r, s, "%s records, update %d, builder %s" % (source, update, builder))
    finally:
        c.close()


@pytest.mark.gpu
def test_refit_then_tlas_update_equals_a_fresh_build():
    import torch
    from tests.test_blas_refit import deform, with_mesh
    parts, sc0, sets, pairs, ref = scene_and_sets("small")
    verts, idx, ranges, inst = parts
    geom = types.SimpleNamespace(verts=verts, idx=idx, ranges=ranges)
    s = np.concatenate([x[:500] for x in sets.values()])
    src = dev(s)
    c, fresh = RtContext(0), RtContext(0)
    try:
        load(c, parts)
        t = deform(geom, 0, amp=0.2)
        torch.cuda.synchronize()
        c.refit_blas_device(0, t)
        torch.cuda.synchronize()
        hits = torch.empty((len(s), 5), dtype=torch.int32, device="cuda:0")
        rc = c.L.rt_sweep_spheres_device(c.h, len(s), ctypes.c_void_p(src.data_ptr()), 0xFF, ctypes.c_void_p(hits.data_ptr()), None, None)
        assert rc == RT_ERR_NOT_READY
        c.set_instances_device(dev_inst(inst))
        v2 = with_mesh(geom, verts, 0, t)
        load(fresh, (v2, idx, ranges, inst))
        got, want = gpu_sweep(c, s)[0], gpu_sweep(fresh, s)[0]
        assert got.tobytes() == want.tobytes()
        check(got, sr.brute32(cr.Scene(v2, idx, ranges, inst), s), s, "after the refit")
    finally:
        c.close()
        fresh.close()


@pytest.mark.gpu
def test_attributes_and_side_words(ctx):
    """d_attr: what rt_closest_point_device writes for the same (inst, prim, u, v) (P, N, objectIndex: bit for bit the oracle's
    hit_attributes of the returned records, which tests/test_closest_point.py holds that call to, and to rounding that call itself at
    the contact point), and the side of the plane the centre lies on at the contact"""
    parts, sc, sets, pairs, ref = scene_and_sets("small")
    load(ctx, parts)
    orc = oracle_scene(*parts)
    for k in ("aimed", "inside", "misc"):
        s = sets[k]
        h, a = gpu_sweep(ctx, s, attributes=True)
        check(h, ref[k], s, "attributes " + k)
        kinds, _ = sr.side_words(sc, s, ref[k])
        assert np.array_equal(a[:, 7].view(np.uint32), kinds), k
        assert set(np.unique(kinds)) == {0, cr.FRONT, cr.BACK}, k
        o = orc.hit_attributes(np.ascontiguousarray(h))
        f = a.view(np.float32)
        assert np.array_equal(f[:, 0:3].view(np.uint32), o[:, 0:3].view(np.uint32)), k
        assert np.array_equal(f[:, 4:7].view(np.uint32), o[:, 3:6].view(np.uint32)), k
        assert np.array_equal(a[:, 3], o[:, 6].astype(np.int32)), k
        # directly against rt_closest_point_device at the contact point P (r_max = 1e-3 of the extent): where it names the same triangle
        # (another one that shares the touched edge or vertex is as near) it recomputes (u, v) from P, so its P and N agree with
        # the sweep's to rounding, and objectIndex exactly
        got = h["inst"] >= 0
        lo, hi = scene_box(sc)
        ext = (hi - lo).max()
        pts = np.concatenate([f[got, 0:3], np.full((got.sum(), 1), 1e-3 * ext, np.float32)], axis=1)
        import torch
        cp = ctx.closest_point_device(torch.from_numpy(np.ascontiguousarray(pts)).to("cuda:0"), attributes=True)
        torch.cuda.synchronize()
        ch, ca = cp.numpy()
        same = (ch["inst"] == h["inst"][got]) & (ch["prim"] == h["prim"][got])
        cf = ca.view(np.float32)
        mag = max(np.abs(lo).max(), np.abs(hi).max())
        assert same.mean() > 0.5 and (ch["inst"] >= 0).all(), (k, same.mean())
        assert np.abs(cf[same, 0:3] - f[got][same, 0:3]).max() <= 1e-5 * mag and np.abs(cf[same, 4:7] - f[got][same, 4:7]).max() <= 1e-3, k
        assert np.array_equal(ca[same, 3], a[got][same, 3]), k
        miss = h["inst"] < 0
        assert miss.any() and (a[miss, 0:3] == 0).all() and (a[miss, 4:7] == 0).all() and (a[miss, 7] == 0).all() and (a[miss, 3] == -1).all(), k
        # the contact normal (p(t) - P) / r has unit length where the sphere was not already touching (radii above 1 % of the extent:
        # the quadratics lose 2^-24 E^2 / r of the radius)
        lo, hi = scene_box(sc)
        far = (h["inst"] >= 0) & (h["t"] > 0) & (s[:, 3] > 0.01 * (hi - lo).max())
        p = s[far, 0:3].astype(np.float64) + h["t"][far, None].astype(np.float64) * s[far, 4:7]
        nrm = np.linalg.norm(p - f[far, 0:3], axis=1) / s[far, 3]
        assert far.sum() > (100 if k == "aimed" else 0) and np.abs(nrm - 1).max() < 1e-2, (k, far.sum(), np.abs(nrm - 1).max())


@pytest.mark.gpu
def test_plumbing(ctx):
    """host form = device form; the counting form returns non-zero counters and identical hits; out= reuse; 1, 63, 64 and 65 records;
    a caller's stream with the records written behind a slow queue and overwritten right after the call; n == 0"""
    import torch
    parts, sc, sets, pairs, ref = scene_and_sets("small")
    load(ctx, parts)
    s, r = sets["aimed"], ref["aimed"]
    hh, st = ctx.sweep_spheres(s)
    check(hh, r, s, "host form")
    assert st.node_visits == 0 and st.tri_tests == 0 and st.bvh_node_bytes > 0 and st.bvh_tri_bytes > 0 and st.ms_trace_closest > 0
    hc, st = ctx.sweep_spheres(s, counting=True)
    check(hc, r, s, "host form, counting")
    assert st.node_visits > 0 and st.tri_tests >= int((r["inst"] >= 0).sum())
    assert ctx.sweep_spheres(s, cull_mask=0)[0]["inst"].max() == -1
    for n in (1, 63, 64, 65):
        check(gpu_sweep(ctx, s[:n])[0], r[:n], s[:n], "%d records" % n)
        check(ctx.sweep_spheres(s[:n])[0], r[:n], s[:n], "%d records, host form" % n)
    # out= reuse
    src = dev(s)
    hits = torch.empty((len(s), 5), dtype=torch.int32, device="cuda:0"); attr = torch.empty((len(s), 8), dtype=torch.int32, device="cuda:0")
    res = ctx.sweep_spheres_device(src, attributes=True, out=(hits, attr))
    assert res.hits.data_ptr() == hits.data_ptr() and res.attr.data_ptr() == attr.data_ptr()
    check(res.numpy()[0], r, s, "out= reuse")
    with pytest.raises(ValueError):
        ctx.sweep_spheres_device(src, out=(hits[:-1], None))
    # stream order: the records are made by a kernel behind a slow queue on a side stream, and overwritten right after the calls
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = slow_queue(torch, 12)
        p = (src + (a[0, 0] != a[0, 0]).to(torch.float32) * 0).contiguous()   # made behind the queue, on the side stream
        r1 = ctx.sweep_spheres_device(p, attributes=True, stream=side)
        r2 = ctx.sweep_spheres_device(p, stream=side)
        p.zero_()
        h1, h2 = r1.hits.clone(), r2.hits.clone()
    side.synchronize()
    for hcopy in (h1, h2):
        check(hcopy.cpu().numpy().view(HIT_DTYPE).reshape(-1), r, s, "stream order")
    # n == 0
    e = ctx.sweep_spheres_device(torch.empty((0, 8), dtype=torch.float32, device="cuda:0"), attributes=True)
    assert e.hits.shape == (0, 5) and e.attr.shape == (0, 8)
    assert len(ctx.sweep_spheres(np.zeros((0, 8), np.float32))[0]) == 0


@pytest.mark.gpu
def test_frame_in_flight_beside_a_sweep_query():
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
        sc = cr.Scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances)
        s = sweep_sets(sc, 300, seed=111)["aimed"]
        src = dev(s)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        slot.trace_async(W, H)
        with torch.cuda.stream(side):
            slow_queue(torch, 4)
            res = base.sweep_spheres_device(src, stream=side)
        during, _ = slot.trace_wait()
        after = base.trace(W, H)[0]
        side.synchronize()
        assert np.array_equal(during.view(np.uint32), before.view(np.uint32))
        assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
        check(res.numpy()[0], sr.brute32(sc, s), s, "beside frames")
    finally:
        slot.close()
        base.close()


def _raw(c, n, sweeps, cull, hits, attr):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_sweep_spheres_device(c.h, n, p(sweeps), cull, p(hits), p(attr), None)


@pytest.mark.gpu
def test_error_statuses():
    import torch
    from tests.test_blas_refit import span
    sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
    sc = cr.Scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances)
    s_np = sweep_sets(sc, 200, seed=121)["aimed"]
    ref = sr.brute32(sc, s_np)
    sw = dev(s_np)
    n = sw.shape[0]
    hits = torch.empty((n + 1, 5), dtype=torch.int32, device="cuda:0")
    attr = torch.empty((n + 1, 8), dtype=torch.int32, device="cuda:0")
    S_, H_, A_ = sw.data_ptr(), hits.data_ptr(), attr.data_ptr()
    c = RtContext(0)

    def err(args, code, text):
        assert _raw(c, *args) == code, args
        msg = c.L.rt_last_error(c.h).decode()
        assert text in msg, (args, msg)

    def ok():
        assert c.sweep_spheres_device(sw).numpy()[0].tobytes() == ref.tobytes()

    try:
        err((n, S_, 0xFF, H_, 0), RT_ERR_NOT_READY, "")   # no geometry
        c.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        err((n, S_, 0xFF, H_, 0), RT_ERR_NOT_READY, "")   # no TLAS
        c.set_instances(sp.instances)
        c.set_uniforms(sp.uniforms)
        ok()
        bad = [((0xFFFFFF00, S_, 0xFF, H_, 0), "too many sweeps"), ((n, S_, 0x100, H_, 0), "cull_mask"), ((n, 0, 0xFF, H_, 0), "null sweep/hit pointers"),
               ((n, S_, 0xFF, 0, 0), "null sweep/hit pointers"), ((n, S_ + 4, 0xFF, H_, 0), "aligned"), ((n, S_, 0xFF, H_ + 2, 0), "aligned"),
               ((n, S_, 0xFF, H_, A_ + 4), "aligned")]
        host_buf = np.zeros((n + 1, 8), np.float32)
        pinned = torch.zeros((n, 8), dtype=torch.float32).pin_memory()
        for ptr in ((host_buf.ctypes.data + 15) & ~15, pinned.data_ptr()):   # (16-byte aligned: only the memory kind is wrong)
            bad += [((n, ptr, 0xFF, H_, 0), "device memory of the context's GPU"), ((n, S_, 0xFF, ptr, 0), "device memory of the context's GPU"),
                    ((n, S_, 0xFF, H_, ptr), "device memory of the context's GPU")]
        for args, text in bad:
            err(args, RT_ERR_INVALID_ARGUMENT, text)
            ok()
        # 4-byte aligned hits that are not 16-byte aligned are fine
        assert _raw(c, n, S_, 0xFF, H_ + 4, 0) == 0
        torch.cuda.synchronize()
        assert hits.view(-1)[1:1 + 5 * n].cpu().numpy().tobytes() == ref.tobytes()
        out = np.zeros(n, HIT_DTYPE)
        P = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        assert c.L.rt_sweep_spheres(c.h, n, None, 0xFF, P(out), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_sweep_spheres(c.h, n, P(s_np), 0xFF, None, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_sweep_spheres(c.h, n, P(s_np), 0x100, P(out), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_sweep_spheres(c.h, 0xFFFFFF00, P(s_np), 0xFF, P(out), 0, None) == RT_ERR_INVALID_ARGUMENT
        ok()
        assert _raw(c, 0, 0, 0xFF, 0, 0) == 0   # n == 0 enqueues nothing and needs no pointers
        with pytest.raises(ValueError):
            c.sweep_spheres_device(sw.cpu())
        with pytest.raises(ValueError):
            c.sweep_spheres_device(torch.zeros((4, 4), dtype=torch.float32, device="cuda:0"))
        with pytest.raises(RtError) as e:
            c.sweep_spheres_device(sw, cull_mask=0x1FF)
        assert e.value.code == RT_ERR_INVALID_ARGUMENT
        ok()
        # not ready: a stale TLAS after a BLAS refit
        ff, nf = span(sp.geom, 1)
        v = torch.from_numpy(sp.geom.verts[ff:ff + nf].copy()).to("cuda:0")
        torch.cuda.synchronize()
        c.refit_blas_device(1, v)
        err((n, S_, 0xFF, H_, 0), RT_ERR_NOT_READY, "")
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
        err((n, S_, 0xFF, H_, 0), RT_ERR_INVALID_ARGUMENT, "trace_variant 0")
        a.set_param("trace_variant", 0)
        a.set_instances(sp.instances)
        ok()
    finally:
        a.close()
