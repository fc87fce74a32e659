"""rt_overlap_triangles_device / rt_overlap_triangles: the triangles of the scene that cut or touch every query triangle.

tests/triangle_overlap_reference.py holds the three references: brute32, the canonical binary32 predicate of include/rt_api.h and
DESIGN.md §5 "Triangle overlaps" restated in numpy over every (query, instance, triangle) pair; brute64, the same seventeen axes in
binary64 on the same binary32 inputs; exact, a rational edge-against-triangle test for lattice inputs.  The CPU part holds brute32 to
brute64 (they may differ only on pairs within REL of the decision boundary, on at most 1 % of the intersecting-or-near pairs of a set)
and all three to each other on the integer lattice without exception; the GPU part holds the library to brute32 bit for bit: counts and
id rows, under every tree the library can build, far from the origin, on degenerate geometry, in every max_ids mode, and through the
plumbing of a device query."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import closest_reference as cr
from tests import overlap_reference as orf
from tests import scenes
from tests import triangle_overlap_reference as trf
from tests.query_reference import REL
from tests.test_closest_point import scene_box, surface_points
from tests.test_overlap_boxes import SCENES, aspect, cancelling_scene, lattice_scene
from tests.test_ray_query import PATHS, dev_inst, slow_queue
from tests.test_ray_query_oracle import use_builder
from vulkan_raytracing_amd import RtContext, api
from vulkan_raytracing_amd.api import RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
RESOLVABLE = {"soup": 1e-2, "sliver": 4e-2}   # (the soup's needles are 1e-4 wide, the slivers 4e-4: a hundred times that, as for boxes)


# ---- scenes and query sets ----------------------------------------------------------------------------------------------------

def as_tris(P):
    """(n, 3, 3) vertices -> (n, 12) records; words 3, 7 and 11 are ignored, so they hold what a vertex may not"""
    P = np.asarray(P, np.float64).reshape(-1, 3, 3)
    q = np.zeros((len(P), 12), np.float32)
    q[:, 0:3] = P[:, 0]; q[:, 4:7] = P[:, 1]; q[:, 8:11] = P[:, 2]
    q[:, 3] = 7.0; q[:, 7] = np.nan; q[:, 11] = np.inf
    return q


def invalid_tris(q):
    """records the contract answers with count 0: a NaN or an infinity in a vertex component (the first 8 of 10 rows)"""
    q = np.array(q[:10], np.float32).copy()
    q[0, 0] = np.nan; q[1, 5] = np.inf; q[2, 10] = -np.inf; q[3, 4] = np.nan; q[4, 8] = np.nan; q[5, [1, 5, 9]] = np.inf
    q[6, trf.COLS] = np.nan; q[7, 2] = -np.inf
    return q


def edges(q):
    """(n, 3) the edge lengths of the records, binary64"""
    q = np.asarray(q, np.float64).reshape(-1, 12)
    P = q[:, trf.COLS].reshape(-1, 3, 3)
    return np.stack([np.linalg.norm(P[:, 1] - P[:, 0], axis=1), np.linalg.norm(P[:, 2] - P[:, 1], axis=1), np.linalg.norm(P[:, 0] - P[:, 2], axis=1)], axis=1)


def with_floor(P, floor):
    """triangles (n, 3, 3) scaled up about their centroid until no edge is below 1.5 floor"""
    e = np.min([np.linalg.norm(P[:, 1] - P[:, 0], axis=1), np.linalg.norm(P[:, 2] - P[:, 1], axis=1), np.linalg.norm(P[:, 0] - P[:, 2], axis=1)], axis=0)
    k = np.maximum(1.0, 1.5 * floor / np.maximum(e, 1e-300))
    c = P.mean(axis=1, keepdims=True)
    return c + (P - c) * k[:, None, None]


def edge_floor(sc, resolvable=0.0):
    lo, hi = scene_box(sc)
    return max(2.0 ** -14 * max(np.abs(lo).max(), np.abs(hi).max()), resolvable)


TIES = 96   # tie-deciding queries of a `features` set: at most a twentieth of its 2 000


def query_sets(sc, tris, seed, n=2000, resolvable=0.0):
    """three sets of 2 000 to 2 200 query triangles: `mixed` (random triangles from a thousandth of the scene size to the whole scene,
    one that spans everything, triangles far outside, invalid records), `surface` (small triangles around surface points), `features`
    (zero-area queries: segments in their three spellings through surface points; and the TIES tie-deciding ones: queries that share a
    vertex or an edge with a scene triangle, lie in its plane, or are a point on it).
    What binary32 can resolve bounds the queries from below: no edge that is not collapsed is under 2^-14 of the largest coordinate nor
    under `resolvable`.  The tie-deciding queries sit on triangles of aspect above 0.01 only."""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(sc)
    c, ext = (lo + hi) / 2, hi - lo
    floor = edge_floor(sc, resolvable)
    fat = np.nonzero(aspect(sc) > 0.01)[0]
    size = ext.max() * 10 ** rng.uniform(-3, 0, (n, 1, 1)) * rng.uniform(0.3, 1.0, (n, 1, 3))
    ctr = c + rng.uniform(-0.55, 0.55, (n, 3)) * ext
    P = with_floor(ctr[:, None] + size * rng.uniform(-0.5, 0.5, (n, 3, 3)), floor)
    span = np.array([[lo - 1, [hi[0] + 1, hi[1] + 1, lo[2] - 1], hi + 1]])
    far = c + rng.choice([-1.0, 1.0], (100, 3)) * ext * rng.uniform(3, 50, (100, 3))
    farP = with_floor(far[:, None] + 0.1 * ext * rng.uniform(-1, 1, (100, 3, 3)), floor)
    mixed = np.concatenate([as_tris(P), as_tris(span), as_tris(farP)])
    mixed = np.concatenate([mixed, invalid_tris(mixed)])
    mixed = mixed[rng.permutation(len(mixed))]
    # (around points of triangles with an area, as for boxes)
    area = np.nonzero(aspect(sc) > 1e-6)[0]
    ka = area[rng.integers(0, len(area), n)]
    uv = rng.dirichlet([1, 1, 1], n)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = uv[:, 0:1] * sc.A[ka] + uv[:, 1:2] * sc.B[ka] + uv[:, 2:3] * sc.C[ka] + d * rng.uniform(0, 1e-3 * ext.max(), (n, 1))
    s = np.maximum(ext.max() * 10 ** rng.uniform(-4, -2, (n, 1, 1)), floor)
    w = rng.normal(size=(n, 3, 3))
    surface = as_tris(with_floor(p[:, None] + s * (w - w.mean(axis=1, keepdims=True)), floor))
    # zero-area queries: segments through surface points, spelt (P, Q, Q), (P, P, Q) and (P, Q, a point between them)
    ns = n - TIES
    ks = area[rng.integers(0, len(area), ns)]
    uv = rng.dirichlet([1, 1, 1], ns)
    mid = uv[:, 0:1] * sc.A[ks] + uv[:, 1:2] * sc.B[ks] + uv[:, 2:3] * sc.C[ks]
    p0, p1 = np.zeros((ns, 3)), np.zeros((ns, 3))
    todo = np.arange(ns)
    dots = tris.A[point_triangles(tris)].astype(np.float64)
    for _ in range(50):
        # (a segment and a scene triangle that is one point have no exact axis but the bounds: binary64 cannot part them, while the
        # rounding residue that the fused cross3 of parallel edges leaves in binary32 is an axis like any other and does, DESIGN.md §5.
        # Such pairs are degenerate_pairs' and are held to brute32 alone; here a segment is drawn again until its bounds hold no such point)
        m = len(todo)
        d = rng.normal(size=(m, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        half = np.maximum(ext.max() * 10 ** rng.uniform(-3, -1, (m, 1)), 4 * floor)
        a0, a1 = mid[todo] - d * half * rng.uniform(0.5, 1.0, (m, 1)), mid[todo] + d * half * rng.uniform(0.5, 1.0, (m, 1))
        p0[todo], p1[todo] = a0.astype(np.float32).astype(np.float64), a1.astype(np.float32).astype(np.float64)
        slo, shi = np.minimum(p0[todo], p1[todo])[:, None], np.maximum(p0[todo], p1[todo])[:, None]
        todo = todo[((dots[None] >= slo) & (dots[None] <= shi)).all(-1).any(-1)]
        if not len(todo):
            break
    assert not len(todo)
    kind = np.arange(ns) % 3
    third = np.where((kind == 0)[:, None], p1, np.where((kind == 1)[:, None], p0, p0 + rng.uniform(0.3, 0.7, (ns, 1)) * (p1 - p0)))
    second = np.where((kind == 1)[:, None], p0, p1)
    third = np.where((kind == 1)[:, None], p1, third)
    seg = np.stack([p0, second, third], axis=1)
    # the tie-deciding ones, on the binary32 vertices the predicate forms
    t = TIES // 4
    k = fat[rng.integers(0, len(fat), 4 * t)]
    long_ab = fat[np.linalg.norm(sc.B[fat] - sc.A[fat], axis=1) >= 1.5 * floor]   # (an edge query has the scene triangle's own edge AB)
    k[t:2 * t] = long_ab[rng.integers(0, len(long_ab), t)]
    # (a point query and a zero-area scene triangle have no exact axis but the bounds either: the point queries sit on vertices that lie
    # in the bounds of no zero-area triangle)
    flat = np.nonzero(tris.finite & (aspect(sc) <= 1e-6))[0]
    clear = fat[~((tris.A[fat][:, None] >= tris.mn[flat][None]) & (tris.A[fat][:, None] <= tris.mx[flat][None])).all(-1).any(-1)]
    k[3 * t:] = clear[rng.integers(0, len(clear), t)]
    r = np.maximum(ext.max() * 10 ** rng.uniform(-3, -1.5, (4 * t, 1)), 2 * floor)
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)   # noqa: E731
    j0, j1, j2, j3 = (slice(i * t, (i + 1) * t) for i in range(4))
    A, B, C = tris.A.astype(np.float64), tris.B.astype(np.float64), tris.C.astype(np.float64)
    o1 = unit(rng.normal(size=(t, 3)))
    o2 = unit(np.cross(o1, rng.normal(size=(t, 3))))   # (at a right angle: the third edge is no shorter than the two at the vertex)
    vertex = np.stack([A[k[j0]], A[k[j0]] + r[j0] * rng.uniform(0.5, 1.0, (t, 1)) * o1, A[k[j0]] + r[j0] * rng.uniform(0.5, 1.0, (t, 1)) * o2], axis=1)
    edge = np.stack([A[k[j1]], B[k[j1]], (A[k[j1]] + B[k[j1]]) / 2 + r[j1] * rng.uniform(0.5, 1.0, (t, 1)) * unit(np.cross(B[k[j1]] - A[k[j1]], rng.normal(size=(t, 3))))], axis=1)
    b = rng.dirichlet([1, 1, 1], (t, 3))
    K = k[j2]
    plane = with_floor(np.stack([b[:, i, 0:1] * A[K] + b[:, i, 1:2] * B[K] + b[:, i, 2:3] * C[K] for i in range(3)], axis=1), floor)
    point = np.stack([A[k[j3]]] * 3, axis=1)
    features = np.concatenate([as_tris(seg), as_tris(vertex), as_tris(edge), as_tris(plane), as_tris(point)])
    return {"mixed": mixed, "surface": surface, "features": features}


def point_triangles(tris):
    """the scene triangles that are one point in the binary32 vertices the predicate forms"""
    return np.nonzero(tris.finite & (tris.A == tris.B).all(-1) & (tris.A == tris.C).all(-1))[0]


def degenerate_pairs(sc, tris, seed=159):
    """zero-area queries beside zero-area scene triangles, which the exact seventeen axes cannot part (brute32 alone decides them, by
    the rounding residues of cross3, and the walk, whose boxes hug the triangle, may not reach a pair that only the bounds hold together:
    DESIGN.md §5): segments in their three spellings and points, through and a little beside every scene triangle that is one point"""
    rng = np.random.default_rng(seed)
    a = np.repeat(tris.A[point_triangles(tris)].astype(np.float64), 6, axis=0)
    d = rng.normal(size=(len(a), 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    beside = np.where((np.arange(len(a)) % 2 == 0)[:, None], 0.0, 0.01) * rng.normal(size=(len(a), 3))
    p0, p1 = (a + beside - 0.3 * d).astype(np.float32).astype(np.float64), (a + beside + 0.5 * d).astype(np.float32).astype(np.float64)
    kind = (np.arange(len(a)) // 2) % 3
    seg = np.stack([p0, np.where((kind == 1)[:, None], p0, p1), np.where((kind == 2)[:, None], p0 + 0.375 * (p1 - p0), p1)], axis=1)
    return np.concatenate([as_tris(seg), as_tris(np.stack([a[::6]] * 3, axis=1))])


def lattice_queries():
    """lattice triangles around lattice_scene: random small ones, and for every third scene triangle (A, B, C) with u = B - A, v = C - A
    the triangle itself, its coplanar mirror over AB (edge-sharing), an edge-sharing one out of the plane, vertex-touching ones in and
    out of the plane, a coplanar one that contains it, a coplanar one beside it, and one through it"""
    rng = np.random.default_rng(173)
    sc = cr.Scene(*lattice_scene())
    T = np.stack([sc.A, sc.B, sc.C], axis=1)[::3]
    A, u, v = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    z = np.array([0.0, 0.0, 1.0])
    parts = [T, np.stack([A, A + u, A + u - v], axis=1), np.stack([A, A + u, A + v + 3 * z], axis=1), np.stack([A + u, A + 2 * u, A + u + v], axis=1),
             np.stack([A, A + [1, 0, 2], A + [0, 1, 2]], axis=1), np.stack([A - u - v, A + 3 * u - v, A - u + 3 * v], axis=1),
             np.stack([A + 3 * u, A + 4 * u, A + 3 * u + v], axis=1), np.stack([A + u + v - 2 * z, A + u + v + 2 * z, A - z], axis=1)]
    base = np.stack([rng.integers(-9, 8, 300), rng.integers(-7, 8, 300), rng.integers(-4, 6, 300)], axis=1)
    parts.append(base[:, None] + rng.integers(-2, 3, (300, 3, 3)))
    P = np.concatenate(parts).astype(np.float64)
    keep = np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1) > 0   # (exact is for non-degenerate triangles)
    return as_tris(P[keep])


_CACHE = {}


def scene_and_sets(name):
    """the scene, its Triangles, its query sets and brute32 of every set at max_ids 16, computed once"""
    if name not in _CACHE:
        from tests.test_closest_point import small_scene
        if name == "lattice":
            parts = lattice_scene()
        elif name == "cancel":
            parts = cancelling_scene()
        elif name.startswith("small+"):
            parts = small_scene(seed=161, offset=float(name[6:]))
        else:
            parts = SCENES[name]()
        sc = cr.Scene(*parts)
        tris = trf.Triangles(sc)
        sets = {"lattice": lattice_queries()} if name == "lattice" else query_sets(sc, tris, seed=153, resolvable=RESOLVABLE.get(name, 0.0))
        ref = {k: trf.brute32(sc, q, tris=tris) for k, q in sets.items()}
        _CACHE[name] = (parts, sc, tris, sets, ref)
    return _CACHE[name]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_exports_abi_and_null_context():
    assert "rt_overlap_triangles_device" in api.EXPORTS and "rt_overlap_triangles" in api.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^int rt_overlap_triangles_device\(rt_ctx\* ctx, size_t n, const void\* d_tris12, uint32_t cull_mask, uint32_t flags,\s+uint32_t max_ids, "
                     r"void\* d_ids, void\* d_counts, void\* hip_stream\);", hdr, re.M)
    assert re.search(r"^int rt_overlap_triangles\(rt_ctx\* ctx, size_t n, const float\* tris12_host, uint32_t cull_mask, uint32_t flags,\s+uint32_t max_ids, "
                     r"int32_t\* ids_host, uint32_t\* counts_host, int counting, rt_stats\* stats\);", hdr, re.M)
    L = api.lib()
    assert hasattr(L, "rt_overlap_triangles_device") and hasattr(L, "rt_overlap_triangles") and L.rt_abi_version() == 7
    assert L.rt_overlap_triangles_device(None, 0, None, 0xFF, 0, 0, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_overlap_triangles_device(None, 64, None, 0xFF, 0, 4, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_overlap_triangles(None, 0, None, 0xFF, 0, 0, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert hasattr(RtContext, "overlap_triangles_device") and hasattr(RtContext, "overlap_triangles") and hasattr(api, "triangle_records")


def test_triangle_records_from_arrays():
    v = np.arange(15, dtype=np.float64).reshape(5, 3)
    f = np.array([[0, 1, 2], [4, 2, 3]], np.uint32)
    r = api.triangle_records(v, f)
    assert r.dtype == np.float32 and r.shape == (2, 12) and (r[:, [3, 7, 11]] == 0).all()
    assert np.array_equal(r[:, trf.COLS].reshape(2, 3, 3), v[f.astype(np.int64)].astype(np.float32))
    assert api.triangle_records(v, np.zeros((0, 3), np.int64)).shape == (0, 12)


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_triangle_kernels_keep_the_record_level_budget(target):
    """exactly two new walk kernels, k_collide_triangles and its counting form, in both libraries, each within the record-level walks'
    budget (>= 4 waves per SIMD, scratch <= 32 bytes, no spills, the 12 KB stack in LDS)"""
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    walk = [(n, r) for n, r in kernels.items() if "k_collide_triangles" in n]
    assert len(walk) == 2 and sum("k_collide_triangles_count" in n for n, _ in walk) == 1, "\n".join(kernels)
    for name, r in walk:
        assert int(r["Occupancy"]) >= 4 and int(r["ScratchSize"]) <= 32 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert int(r["LDS Size"]) == 12288, (name, r)


def test_the_query_sets_are_what_they_claim():
    """no edge that is not collapsed under 2^-14 of the largest coordinate or under the resolvable floor; at most a twentieth of a
    features set decides on ties; the invalid records are invalid"""
    for name in ("small", "teapot", "soup", "sliver", "small+1000", "small+10000", "cancel"):
        parts, sc, tris, sets, ref = scene_and_sets(name)
        floor = edge_floor(sc, RESOLVABLE.get(name, 0.0))
        for k, q in sets.items():
            e = edges(q[trf.valid_queries(q)])
            assert e[e > 0].min() >= floor, (name, k, e[e > 0].min(), floor)
            assert 2000 <= len(q) <= 2200
        assert TIES <= len(sets["features"]) // 20
        assert (~trf.valid_queries(sets["mixed"])).sum() == 8
        e = np.sort(edges(sets["features"][:len(sets["features"]) - TIES]), axis=1)   # the zero-area queries: the short edges make the long one
        assert (np.abs(e[:, 0] + e[:, 1] - e[:, 2]) <= 1e-6 * e[:, 2]).all()


@pytest.mark.parametrize("name", ["small", "teapot", "soup", "sliver", "small+1000", "small+10000", "cancel"])
def test_binary32_restatement_against_binary64(name):
    """every pair on which brute32 and brute64 disagree has a binary64 separation within REL of zero, and such pairs are at most 1 % of
    the set's intersecting-or-near pairs (binary64 candidates and pairs separated by at most REL).  Every set of every scene of the GPU
    tests."""
    parts, sc, tris, sets, ref = scene_and_sets(name)
    for k, q in sets.items():
        qi, ti = trf.surviving_pairs(tris, q)
        c32 = trf.candidates32(tris, q, qi, ti)
        s64 = trf.separation64(tris, q, qi, ti)
        differ = c32 != (s64 <= 0)
        near = np.abs(s64) <= REL
        pool = (s64 <= 0) | near
        print("%s %s: %d pairs past the bounds axes, %d intersecting or near, %d near, %d differ (worst |separation| %.3g)" %
              (name, k, len(qi), pool.sum(), near.sum(), differ.sum(), np.abs(s64[differ]).max() if differ.any() else 0.0))
        assert (ref[k][0] == np.bincount(qi[c32], minlength=len(q))).all()
        assert near[differ].all(), (k, np.abs(s64[differ]).max())
        assert differ.sum() <= 0.01 * pool.sum(), (k, differ.sum(), pool.sum())


def test_the_integer_lattice_is_exact():
    """brute32, brute64 and the rational test agree on every pair, with no exception: lattice triangles that coincide with scene
    triangles, share an edge or a vertex with them in and out of their plane, contain them, lie beside them in their plane, cross them.
    Every candidate is a candidate of the box predicate for the query's bounds."""
    parts, sc, tris, sets, ref = scene_and_sets("lattice")
    q = sets["lattice"]
    qi, ti = trf.surviving_pairs(tris, q)
    c32 = trf.candidates32(tris, q, qi, ti)
    s64 = trf.separation64(tris, q, qi, ti)
    ex = trf.exact(tris, q, qi, ti)
    print("lattice: %d queries, %d pairs past the bounds axes, %d candidates, %d touching (separation 0)" % (len(q), len(qi), c32.sum(), (s64 == 0).sum()))
    assert np.array_equal(c32, s64 <= 0) and np.array_equal(c32, ex)
    assert c32.sum() > 1000 and (~c32).sum() > 1000 and (s64 == 0).sum() > 300
    box = orf.candidates32(tris, trf.bounds(q), qi, ti)
    assert (box | ~c32).all() and (box & ~c32).any()
    r64 = trf.brute64(sc, q, tris=tris)
    assert r64[0].tobytes() == ref["lattice"][0].tobytes() and r64[1].tobytes() == ref["lattice"][1].tobytes()


def test_restatement_edge_cases():
    """invalid records, cull masks, a point query, a segment query, a zero-area scene triangle, identical triangles, a query equal to a
    scene triangle: brute32 alone"""
    parts, sc, tris, sets, ref = scene_and_sets("small")
    bad = invalid_tris(sets["surface"])
    assert not trf.valid_queries(bad)[:8].any() and trf.valid_queries(bad)[8:].all()
    counts, ids = trf.brute32(sc, bad, tris=tris)
    assert (counts[:8] == 0).all() and (ids[:8] == -1).all()
    assert (trf.brute32(sc, sets["mixed"], 0, tris=tris)[0] == 0).all()
    # a query equal to a scene triangle (the binary32 vertices the predicate forms) finds it, under every admitting mask only
    k = np.nonzero(sc.admitted(0xFF))[0][::7]
    own = np.stack([sc.inst[k], sc.prim[k]], axis=1)
    same = as_tris(np.stack([tris.A[k], tris.B[k], tris.C[k]], axis=1))
    counts, ids = trf.brute32(sc, same, tris=tris)
    assert (counts >= 1).all() and all((ids[i] == own[i]).all(axis=1).any() for i in range(len(k)))
    counts, ids = trf.brute32(sc, same, 0x01, tris=tris)
    adm = sc.admitted(0x01)[k]
    assert all((ids[i] == own[i]).all(axis=1).any() == adm[i] for i in range(len(k)))
    # identical queries give identical rows; a rotation of the vertices names the same triangle and here the same candidates
    twice = np.concatenate([same, same])
    c2, i2 = trf.brute32(sc, twice, tris=tris)
    assert np.array_equal(c2[:len(k)], c2[len(k):]) and np.array_equal(i2[:len(k)], i2[len(k):])
    # a point query on a vertex finds the triangles that hold it as their A; 50 units away it finds nothing
    at = as_tris(np.stack([tris.A[k]] * 3, axis=1))
    counts, ids = trf.brute32(sc, at, tris=tris)
    assert (counts >= 1).all() and all((ids[i] == own[i]).all(axis=1).any() for i in range(len(k)))
    assert (trf.brute32(sc, as_tris(np.stack([tris.A[k] + 50.0] * 3, axis=1)), tris=tris)[0] == 0).all()
    # a segment query through a triangle's centroid along its normal finds it, in each spelling; one that stops short does not
    A, B, C = (x[k].astype(np.float64) for x in (tris.A, tris.B, tris.C))
    g = (A + B + C) / 3
    nrm = np.cross(B - A, C - A); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    for P in ([g - nrm, g + nrm, g + nrm], [g - nrm, g - nrm, g + nrm], [g - nrm, g + nrm, g + 0.25 * nrm]):
        counts, ids = trf.brute32(sc, as_tris(np.stack(P, axis=1)), tris=tris)
        assert all((ids[i] == own[i]).all(axis=1).any() for i in range(len(k)))
    counts, ids = trf.brute32(sc, as_tris(np.stack([g + 0.5 * nrm, g + nrm, g + nrm], axis=1)), max_ids=64, tris=tris)
    assert not any((ids[i] == own[i]).all(axis=1).any() for i in range(len(k)))
    # zero-area scene triangles (a, a, a): a query through the point finds them (their axes are zero and separate nothing)
    parts, sc, tris, sets, ref = scene_and_sets("soup")
    deg = np.nonzero((sc.prim % 6 == 3) & sc.admitted(0xFF))[0]
    a = tris.A[deg].astype(np.float64)
    through = as_tris(np.stack([a + [1, 0, 0], a + [-1, 1, 0], a + [-1, -1, 0]], axis=1))
    counts, ids = trf.brute32(sc, through, max_ids=64, tris=tris)
    own = np.stack([sc.inst[deg], sc.prim[deg]], axis=1)
    assert all((ids[i] == own[i]).all(axis=1).any() for i in range(len(deg)))
    assert (trf.brute32(sc, as_tris(np.stack([a + 50, a + [51, 50, 50], a + [50, 51, 50]], axis=1)), tris=tris)[0] == 0).all()
    # zero-area queries beside them: the point query on the point finds it, whatever else the residues decide
    dq = degenerate_pairs(sc, tris)
    pts = point_triangles(tris)
    counts, ids = trf.brute32(sc, dq, max_ids=64, tris=tris)
    own = np.stack([sc.inst[pts], sc.prim[pts]], axis=1)
    assert len(pts) >= 8 and all((ids[6 * len(pts) + i] == own[i]).all(axis=1).any() for i in np.nonzero(sc.admitted(0xFF)[pts])[0])


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


def dev(q):
    import torch
    return torch.from_numpy(np.ascontiguousarray(q, np.float32).reshape(-1, 12)).to("cuda:0")


def gpu_overlap(c, q, max_ids=16, cull=0xFF, counts=True, any=False):
    import torch
    res = c.overlap_triangles_device(dev(q), max_ids=max_ids, cull_mask=cull, counts=counts, any=any)
    torch.cuda.synchronize()
    return res.numpy()


def check(got, ref, what, max_ids=16):
    """(counts, ids) of the GPU against brute32's at max_ids 16, bit for bit"""
    counts, ids = got
    rc, ri = ref
    if counts is not None and counts.tobytes() != rc.tobytes():
        bad = np.nonzero(counts != rc)[0]
        raise AssertionError("%s: %d counts differ from the brute force, first query %d: gpu %d reference %d" % (what, len(bad), bad[0], counts[bad[0]], rc[bad[0]]))
    if max_ids:
        want = np.ascontiguousarray(ri[:, :max_ids])
        if ids.tobytes() != want.tobytes():
            bad = np.nonzero((ids != want).any(axis=(1, 2)))[0]
            raise AssertionError("%s: %d rows differ from the brute force, first query %d: gpu %s reference %s" % (what, len(bad), bad[0], ids[bad[0]].tolist(), want[bad[0]].tolist()))
    else:
        assert ids is None, what


def load(c, parts):
    verts, idx, ranges, inst = parts
    c.upload_geometry(verts, idx, ranges)
    c.set_instances(inst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "teapot", "soup", "sliver"])
def test_every_query_set(ctx, name):
    """random triangles of every size, small ones on the surface, zero-area and tie-deciding ones, the one that spans everything,
    triangles far outside, invalid records; cull masks"""
    parts, sc, tris, sets, ref = scene_and_sets(name)
    load(ctx, parts)
    for k, q in sets.items():
        check(gpu_overlap(ctx, q), ref[k], "%s %s" % (name, k))
    mixed = sets["mixed"]
    if len(point_triangles(tris)):
        # two zero-area triangles that only their bounds hold together: the library lists candidates of the predicate only, and a point
        # query on a scene triangle that is that point finds it
        dq = degenerate_pairs(sc, tris)
        pts = point_triangles(tris)
        rc, ri = trf.brute32(sc, dq, max_ids=64, tris=tris)
        assert rc.max() <= 64
        gc, gi = gpu_overlap(ctx, dq)
        assert (gc <= rc).all() and (gc <= 16).all()
        for i in range(len(dq)):
            assert {tuple(x) for x in gi[i, :gc[i]]} <= {tuple(x) for x in ri[i, :rc[i]]}, (name, i)
        for i in np.nonzero(sc.admitted(0xFF)[pts])[0]:
            assert (gi[6 * len(pts) + i] == [sc.inst[pts[i]], sc.prim[pts[i]]]).all(axis=1).any(), (name, i)
    assert (ref["mixed"][0][~trf.valid_queries(mixed)] == 0).all() and ref["mixed"][0].max() >= 12 and (ref["features"][0] > 0).mean() > 0.5
    for cull in (0x01, 0x5A, 0x00):
        check(gpu_overlap(ctx, mixed, cull=cull), trf.brute32(sc, mixed, cull, tris=tris), "%s mixed cull %#x" % (name, cull))


@pytest.mark.gpu
def test_the_integer_lattice(ctx):
    """coinciding, edge-sharing, vertex-touching, containing and crossing lattice triangles: closed sets, exact answers"""
    parts, sc, tris, sets, ref = scene_and_sets("lattice")
    load(ctx, parts)
    q = sets["lattice"]
    check(gpu_overlap(ctx, q), ref["lattice"], "lattice")
    occ = gpu_overlap(ctx, q, max_ids=0, any=True)[0]
    assert np.array_equal(occ, (ref["lattice"][0] > 0).astype(np.uint32))


@pytest.mark.gpu
def test_max_ids_counts_pruning_and_any(ctx):
    """max_ids 0, 1, 3, 16 on queries with more candidates than that, with and without counts (the pruning path): the same rows;
    RT_OVERLAP_ANY equals count > 0"""
    parts, sc, tris, sets, ref = scene_and_sets("teapot")   # (a plane cuts fewer triangles than a box holds: the finer mesh)
    load(ctx, parts)
    rc, ri = ref["mixed"]
    many = np.nonzero(rc > 16)[0]
    assert len(many) >= 30
    q = np.concatenate([sets["mixed"][many], sets["mixed"][:500]])
    r = (np.concatenate([rc[many], rc[:500]]), np.concatenate([ri[many], ri[:500]]))
    for k in (0, 1, 3, 16):
        check(gpu_overlap(ctx, q, max_ids=k), r, "max_ids %d with counts" % k, max_ids=k)
        if k:
            counts, ids = gpu_overlap(ctx, q, max_ids=k, counts=False)
            assert counts is None
            check((None, ids), r, "max_ids %d without counts" % k, max_ids=k)
    for name, b in sets.items():
        occ, ids = gpu_overlap(ctx, b, max_ids=0, any=True)
        assert ids is None and np.array_equal(occ, (ref[name][0] > 0).astype(np.uint32)), name
    occ = gpu_overlap(ctx, q, max_ids=0, any=True, cull=0x02)[0]
    assert np.array_equal(occ, (trf.brute32(sc, q, 0x02, tris=tris)[0] > 0).astype(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "unset", "1", "2"])
def test_tree_independence(builder, monkeypatch):
    """the same queries over blas_builder 0 and RT_GPU_BVH_ALGO unset / 1 / 2, host and device instance records with their refits: every
    output equals one brute force, so they are byte-identical to each other"""
    import torch
    parts, sc0, tris0, sets, ref = scene_and_sets("small")
    verts, idx, ranges, inst = parts
    rng = np.random.default_rng(72)
    moved = inst.copy()
    moved["transform"][:, [3, 7, 11]] += rng.uniform(-0.3, 0.3, (len(inst), 3)).astype(np.float32)
    q = np.concatenate([sets["mixed"][:1200], sets["surface"][:600], sets["features"][-600:]])
    r0 = tuple(np.concatenate([ref["mixed"][j][:1200], ref["surface"][j][:600], ref["features"][j][-600:]]) for j in (0, 1))
    r1 = trf.brute32(cr.Scene(verts, idx, ranges, moved), q)
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
                what = "%s records, update %d, builder %s" % (source, update, builder)
                check(gpu_overlap(c, q), r, what)
                check(gpu_overlap(c, q, max_ids=3, counts=False), r, what + ", pruning", max_ids=3)
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small+1000", "small+10000", "cancel"])
def test_translated_and_cancelling_scenes(ctx, name):
    """the scene 1 000 and 10 000 units from the origin, and instances whose translation cancels their mesh's own offset: the walk's
    slack must cover the rounding of the world vertices"""
    parts, sc, tris, sets, ref = scene_and_sets(name)
    load(ctx, parts)
    for k, q in sets.items():
        check(gpu_overlap(ctx, q), ref[k], "%s %s" % (name, k))
    assert (ref["surface"][0] > 0).mean() > 0.5


@pytest.mark.gpu
def test_refit_then_tlas_update_equals_a_fresh_build():
    import torch
    from tests.test_blas_refit import deform, with_mesh
    parts, sc0, tris0, sets, ref = scene_and_sets("small")
    verts, idx, ranges, inst = parts
    geom = types.SimpleNamespace(verts=verts, idx=idx, ranges=ranges)
    q = np.concatenate([sets["mixed"][:1500], sets["surface"][:800]])
    src = dev(q)
    c, fresh = RtContext(0), RtContext(0)
    try:
        load(c, parts)
        t = deform(geom, 0, amp=0.2)
        torch.cuda.synchronize()
        c.refit_blas_device(0, t)
        torch.cuda.synchronize()
        ids = torch.empty((len(q), 16, 2), dtype=torch.int32, device="cuda:0")
        rc = c.L.rt_overlap_triangles_device(c.h, len(q), ctypes.c_void_p(src.data_ptr()), 0xFF, 0, 16, ctypes.c_void_p(ids.data_ptr()), None, None)
        assert rc == RT_ERR_NOT_READY
        c.set_instances_device(dev_inst(inst))
        v2 = with_mesh(geom, verts, 0, t)
        load(fresh, (v2, idx, ranges, inst))
        got, want = gpu_overlap(c, q), gpu_overlap(fresh, q)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        check(got, trf.brute32(cr.Scene(v2, idx, ranges, inst), q), "after the refit")
    finally:
        c.close()
        fresh.close()


@pytest.mark.gpu
def test_self_collision_through_the_cull_mask(ctx):
    """the instances of the small scene pulled together until they interpenetrate; the world triangles of one of them, built on the
    device with api.triangle_records from its mesh and transform, against the others: that instance has a mask bit of its own and the
    call's cull mask leaves it out"""
    import torch
    from tests.test_closest_point import small_scene
    verts, idx, ranges, inst = small_scene(seed=157)
    inst = inst.copy()
    inst["transform"][:, [3, 7, 11]] *= np.float32(0.3)
    me = 5
    for i in range(len(inst)):
        inst[i]["custom_index_and_mask"] = (int(inst[i]["custom_index_and_mask"]) & 0xFFFFFF) | ((0x01 if i == me else 0x02) << 24)
    load(ctx, (verts, idx, ranges, inst))
    ff, fi, pc = ranges[int(inst[me]["mesh"])]
    faces = torch.from_numpy(np.asarray(idx[fi:fi + 3 * pc], np.int64).reshape(-1, 3)).to("cuda:0")
    v = torch.from_numpy(np.asarray(verts, np.float32)[ff:].reshape(-1, 6)[:, :3].copy()).to("cuda:0")
    M = torch.from_numpy(np.asarray(inst[me]["transform"], np.float32).reshape(3, 4)).to("cuda:0")
    q = api.triangle_records(v @ M[:, :3].T + M[:, 3], faces)
    assert q.is_cuda and q.shape == (pc, 12) and q.dtype == torch.float32 and q.is_contiguous()
    res = ctx.overlap_triangles_device(q, max_ids=16, cull_mask=0x02)
    torch.cuda.synchronize()
    sc = cr.Scene(verts, idx, ranges, inst)
    qn = q.cpu().numpy()
    r = trf.brute32(sc, qn, 0x02)
    check(res.numpy(), r, "self-collision")
    assert (r[0] > 0).sum() >= 3 and (r[1][..., 0] != me).all()
    # with its own bit admitted every triangle finds at least itself
    both = trf.brute32(sc, qn, 0x03)
    check(gpu_overlap(ctx, qn, cull=0x03), both, "with its own instance")
    assert (both[0] > r[0]).all()


@pytest.mark.gpu
def test_counters_equal_the_box_walk_on_the_bounds(ctx):
    """with counts requested nothing prunes: the node test is the box query's on the queries' bounds and packets are counted before the
    test, so node_visits and tri_tests equal rt_overlap_boxes' exactly"""
    for name in ("small", "sliver"):
        parts, sc, tris, sets, ref = scene_and_sets(name)
        load(ctx, parts)
        for k, q in sets.items():
            cnt, ids, st = ctx.overlap_triangles(q, max_ids=16, counting=True)
            check((cnt, ids), ref[k], "%s %s, counting" % (name, k))
            bc, _, sb = ctx.overlap_boxes(trf.bounds(q), max_ids=16, counting=True)
            assert st.node_visits == sb.node_visits > 0 and st.tri_tests == sb.tri_tests >= int(bc.sum()), (name, k)


@pytest.mark.gpu
def test_plumbing(ctx):
    """a caller's stream with the records written by a kernel queued just before the call; out= reuse; host form = device form; counting
    fills the visit counters; n == 0"""
    import torch
    parts, sc, tris, sets, ref = scene_and_sets("small")
    load(ctx, parts)
    q = sets["mixed"]
    r = ref["mixed"]
    # host form
    cnt, ids, st = ctx.overlap_triangles(q, max_ids=16)
    check((cnt, ids), r, "host form")
    assert st.node_visits == 0 and st.tri_tests == 0 and st.ms_trace_closest > 0 and st.bvh_node_bytes == 32 and st.bvh_tri_bytes == 48
    cnt, ids, st = ctx.overlap_triangles(q, max_ids=16, counting=True)
    check((cnt, ids), r, "host form, counting")
    assert st.node_visits > 0 and st.tri_tests >= int(r[0].sum())
    cnt, ids, st = ctx.overlap_triangles(q, max_ids=0, counting=True)
    assert ids is None and cnt.tobytes() == r[0].tobytes()
    cnt, ids, st_any = ctx.overlap_triangles(q, max_ids=0, any=True, counting=True)
    assert np.array_equal(cnt, (r[0] > 0).astype(np.uint32)) and 0 < st_any.tri_tests <= st.tri_tests
    cnt, ids, _ = ctx.overlap_triangles(q, max_ids=3, counts=False)
    assert cnt is None
    check((None, ids), r, "host form without counts", max_ids=3)
    # out= reuse
    src = dev(q)
    ids_t = torch.empty((len(q), 16, 2), dtype=torch.int32, device="cuda:0"); cnt_t = torch.empty((len(q),), dtype=torch.int32, device="cuda:0")
    res = ctx.overlap_triangles_device(src, max_ids=16, out=(ids_t, cnt_t))
    assert res.ids.data_ptr() == ids_t.data_ptr() and res.count.data_ptr() == cnt_t.data_ptr() and isinstance(res, api.BoxOverlaps)
    check(res.numpy(), r, "out= reuse")
    assert res.inst.shape == (len(q), 16) and res.prim.shape == (len(q), 16)
    with pytest.raises(ValueError):
        ctx.overlap_triangles_device(src, max_ids=16, out=(ids_t[:-1], cnt_t))
    # stream order: the records are made by a kernel behind a slow queue on a side stream, and overwritten right after the call
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = slow_queue(torch, 12)
        p = (src + (a[0, 0] != a[0, 0]).to(torch.float32) * 0).contiguous()   # made behind the queue, on s
        r1 = ctx.overlap_triangles_device(p, max_ids=16, stream=s)
        r2 = ctx.overlap_triangles_device(p, max_ids=0, any=True, stream=s)
        p.zero_()
        i1, c1, c2 = r1.ids.clone(), r1.count.clone(), r2.count.clone()
    s.synchronize()
    check((c1.cpu().numpy().view(np.uint32), i1.cpu().numpy()), r, "stream order")
    assert np.array_equal(c2.cpu().numpy().view(np.uint32), (r[0] > 0).astype(np.uint32))
    # n == 0
    e = ctx.overlap_triangles_device(torch.empty((0, 12), dtype=torch.float32, device="cuda:0"), max_ids=4)
    assert e.ids.shape == (0, 4, 2) and e.count.shape == (0,)
    cnt, ids, _ = ctx.overlap_triangles(np.zeros((0, 12), np.float32), max_ids=2)
    assert len(cnt) == 0 and ids.shape == (0, 2, 2)


@pytest.mark.gpu
def test_frame_in_flight_and_a_second_slot():
    """a frame in flight on a second slot is neither waited for nor changed by a query on the root: its pixels equal the frame rendered
    alone; the slot answers the query over its own instances as the root does"""
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
        rng = np.random.default_rng(111)
        p = surface_points(sc, 2000, rng, 0.0)
        lo, hi = scene_box(sc)
        h = (hi - lo).max() * 10 ** rng.uniform(-3, -1.5, (2000, 1, 1))
        q = as_tris(p[:, None] + h * rng.uniform(-1, 1, (2000, 3, 3)))
        src = dev(q)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        slot.trace_async(W, H)
        with torch.cuda.stream(s):
            slow_queue(torch, 4)
            res = base.overlap_triangles_device(src, max_ids=16, stream=s)
        during, _ = slot.trace_wait()
        after = base.trace(W, H)[0]
        s.synchronize()
        assert np.array_equal(during.view(np.uint32), before.view(np.uint32))
        assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
        r = trf.brute32(sc, q)
        check(res.numpy(), r, "beside frames")
        check(gpu_overlap(slot, q), r, "on the second slot")
    finally:
        slot.close()
        base.close()


def _raw(c, n, tris, cull, flags, k, ids, counts):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_overlap_triangles_device(c.h, n, p(tris), cull, flags, k, p(ids), p(counts), None)


@pytest.mark.gpu
def test_error_statuses():
    import torch
    from tests.test_blas_refit import span
    sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
    sc = cr.Scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances)
    rng = np.random.default_rng(121)
    pts = surface_points(sc, 500, rng, 0.0)
    q_np = as_tris(pts[:, None] + 0.02 * rng.uniform(-1, 1, (500, 3, 3)))
    ref = trf.brute32(sc, q_np, max_ids=4)
    q = dev(q_np)
    n = q.shape[0]
    ids = torch.empty((n + 1, 4, 2), dtype=torch.int32, device="cuda:0")
    cnt = torch.empty((n + 1,), dtype=torch.int32, device="cuda:0")
    B_, I_, C_ = q.data_ptr(), ids.data_ptr(), cnt.data_ptr()
    c = RtContext(0)

    def err(args, code, text):
        assert _raw(c, *args) == code, args
        msg = c.L.rt_last_error(c.h).decode()
        assert text in msg, (args, msg)

    def ok():
        got = c.overlap_triangles_device(q, max_ids=4).numpy()
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()

    try:
        err((n, B_, 0xFF, 0, 4, I_, C_), RT_ERR_NOT_READY, "")   # no geometry
        c.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        err((n, B_, 0xFF, 0, 4, I_, C_), RT_ERR_NOT_READY, "")   # no TLAS
        c.set_instances(sp.instances)
        c.set_uniforms(sp.uniforms)
        ok()
        bad = [((0xFFFFFF00, B_, 0xFF, 0, 4, I_, C_), "too many triangles"), ((0x10000000, B_, 0xFF, 0, 16, I_, C_), "n * max_ids"),
               ((n, B_, 0x100, 0, 4, I_, C_), "cull_mask"), ((n, B_, 0xFF, 0x2, 4, I_, C_), "unknown flag bits"), ((n, B_, 0xFF, 0x80000000, 0, 0, C_), "unknown flag bits"),
               ((n, B_, 0xFF, 0, 17, I_, C_), "max_ids must be 0..16"), ((n, B_, 0xFF, 0, 0, I_, C_), "max_ids 0 counts only"), ((n, B_, 0xFF, 0, 0, I_, 0), "max_ids 0 counts only"),
               ((n, B_, 0xFF, 1, 4, I_, C_), "RT_OVERLAP_ANY needs max_ids 0"), ((n, B_, 0xFF, 1, 0, 0, 0), "neither ids nor counts"),
               ((n, B_, 0xFF, 0, 4, 0, 0), "neither ids nor counts"), ((n, B_, 0xFF, 0, 4, 0, C_), "null id pointer"), ((n, 0, 0xFF, 0, 4, I_, C_), "null triangle pointer"),
               ((n, B_ + 4, 0xFF, 0, 4, I_, C_), "aligned"), ((n, B_, 0xFF, 0, 4, I_ + 2, C_), "aligned"), ((n, B_, 0xFF, 0, 4, I_, C_ + 1), "aligned")]
        host_buf = np.zeros((n + 1, 12), np.float32)
        pinned = torch.zeros((n, 12), dtype=torch.float32).pin_memory()
        for ptr in ((host_buf.ctypes.data + 15) & ~15, pinned.data_ptr()):   # (16-byte aligned: only the memory kind is wrong)
            bad += [((n, ptr, 0xFF, 0, 4, I_, C_), "triangles, ids and counts must be device memory of the context's GPU"),
                    ((n, B_, 0xFF, 0, 4, ptr, C_), "device memory of the context's GPU"), ((n, B_, 0xFF, 0, 4, I_, ptr), "device memory of the context's GPU")]
        for args, text in bad:
            err(args, RT_ERR_INVALID_ARGUMENT, text)
            assert "rt_overlap_triangles_device" in c.L.rt_last_error(c.h).decode()
            ok()
        # 4-byte aligned rows and counts that are not 8- or 16-byte aligned are fine
        assert _raw(c, n, B_, 0xFF, 0, 4, I_ + 4, C_ + 4) == 0
        torch.cuda.synchronize()
        assert ids.view(-1)[1:1 + 8 * n].cpu().numpy().tobytes() == ref[1].tobytes() and cnt[1:].cpu().numpy().view(np.uint32).tobytes() == ref[0].tobytes()
        out_c = np.zeros(n, np.uint32)
        P = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        assert c.L.rt_overlap_triangles(c.h, n, None, 0xFF, 0, 0, None, P(out_c), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert "null triangle pointer" in c.L.rt_last_error(c.h).decode()
        assert c.L.rt_overlap_triangles(c.h, n, P(q_np), 0x100, 0, 0, None, P(out_c), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_overlap_triangles(c.h, n, P(q_np), 0xFF, 1, 2, None, P(out_c), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_overlap_triangles(c.h, n, P(q_np), 0xFF, 0, 0, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
        ok()
        assert _raw(c, 0, 0, 0xFF, 0, 0, 0, C_) == 0   # n == 0 enqueues nothing and needs no record pointer
        with pytest.raises(ValueError):
            c.overlap_triangles_device(q.cpu())
        with pytest.raises(ValueError):
            c.overlap_triangles_device(torch.zeros((4, 8), dtype=torch.float32, device="cuda:0"))
        with pytest.raises(ValueError):
            c.overlap_triangles_device(q, max_ids=2, any=True)
        with pytest.raises(ValueError):
            c.overlap_triangles_device(q, max_ids=0, counts=False)
        with pytest.raises(RtError) as e:
            c.overlap_triangles_device(q, cull_mask=0x1FF)
        assert e.value.code == RT_ERR_INVALID_ARGUMENT
        ok()
        # not ready: a stale TLAS after a BLAS refit
        ff, nf = span(sp.geom, 1)
        v = torch.from_numpy(sp.geom.verts[ff:ff + nf].copy()).to("cuda:0")
        torch.cuda.synchronize()
        c.refit_blas_device(1, v)
        err((n, B_, 0xFF, 0, 4, I_, C_), RT_ERR_NOT_READY, "")
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
        err((n, B_, 0xFF, 0, 4, I_, C_), RT_ERR_INVALID_ARGUMENT, "trace_variant 0")
        a.set_param("trace_variant", 0)
        a.set_instances(sp.instances)
        ok()
    finally:
        a.close()


def corridor_triangles():
    """query triangles whose bounds are test_stack_spill's corridor boxes: the plane through a box's main diagonal, which cuts the
    squares of the corridor the box covers.  Returns (tris12, the boxes, target or -1, target of the whole-corridor ones or -2)"""
    from tests.test_stack_spill import S_ROT0, S_ROT1, S_SHEAR, S_TOP, corridor_boxes
    boxes, tag, whole = corridor_boxes((0, S_TOP, S_ROT0, S_ROT1, S_SHEAR), 4, seed=19)
    lo, hi = boxes[:, 0:3].astype(np.float64), boxes[:, 4:7].astype(np.float64)
    P = np.stack([lo, hi, np.stack([lo[:, 0], hi[:, 1], hi[:, 2]], axis=1)], axis=1)
    return as_tris(P), boxes, tag, whole


@pytest.mark.gpu
def test_the_spill_half_of_the_stack():
    """k_collide_triangles on scenes.corridor: the box-overlap order (child 0 first) applies to the queries' bounds, so the modelled
    peak of a query that spans a deep corridor exceeds the 12 entries the LDS holds (asserted on the context's snapshot)"""
    import torch
    from tests import stack_reference as sr
    from tests.test_stack_spill import PLACED_SMALL, S_ROT0, S_ROT1, S_SHEAR, S_TOP, World, premise
    q, boxes, tag, whole = corridor_triangles()
    assert np.array_equal(trf.bounds(q)[:, [0, 1, 2, 4, 5, 6]], boxes[:, [0, 1, 2, 4, 5, 6]])
    w = World(placed=PLACED_SMALL)
    try:
        bq = [sr.Box(b[0:3], b[4:7]) for b in boxes.astype(np.float64)]
        premise(w.model, bq, whole, (S_TOP, S_ROT0, S_ROT1, S_SHEAR), sample=3, what="triangle overlaps")
        sc = cr.Scene(w.verts, w.idx, w.ranges, w.inst)
        rc, ri = trf.brute32(sc, q)
        assert rc.max() >= 1000 and (rc[tag == -1] == 0).all() and (rc[whole >= 0] > 16).all()

        def run(**kw):
            res = w.ctx.overlap_triangles_device(dev(q), **kw)
            torch.cuda.synchronize()
            return res.numpy()

        counts, ids = run(max_ids=16)
        assert counts.tobytes() == rc.tobytes() and ids.tobytes() == ri.tobytes()
        counts, ids = run(max_ids=3, counts=False)
        assert counts is None and ids.tobytes() == np.ascontiguousarray(ri[:, :3]).tobytes()
        occ, ids = run(max_ids=0, any=True)
        assert ids is None and np.array_equal(occ, (rc > 0).astype(np.uint32))
    finally:
        w.ctx.close()
