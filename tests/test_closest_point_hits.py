"""rt_closest_point_device_hits / rt_closest_point_hits: the K nearest triangles of every query point in (d2, inst, prim) order and the
number of triangles within the point's radius.

tests/closest_hits_reference.py holds the reference: brute32_k, the canonical binary32 d2 of tests/closest_reference.py over every
admitted triangle, sorted.  The CPU part holds it to closest_reference.brute32 (its first entry) and to the binary64 distances; the GPU
part holds the library to it byte for byte: rows and counts, with and without counts (the pruned walk), radius classes around K, ties
under every tree producer, cull masks and bad instance records, invalid points, degenerate and far geometry, attributes, the spill half
of the stack, more points than the resident grid has threads, and the plumbing of a device query."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import closest_hits_reference as chr_
from tests import closest_reference as cr
from tests import instance_record_cases as irc
from tests import scenes
from tests.test_closest_point import degenerate_soup, dev, feature_points, invalid_records, load, point_sets, small_scene
from tests.test_ray_query import PATHS, dev_inst, slow_queue
from tests.test_ray_query_oracle import oracle_scene, placed_instances, use_builder
from tests.test_stack_spill import closest_points_and_reference, closest_premise
from tests.test_stack_spill import small as corridors   # noqa: F401 (the corridor world, as a fixture of this module)
from vulkan_raytracing_amd import RtContext, api, host
from vulkan_raytracing_amd.api import HIT_DTYPE, INSTANCE_DTYPE, RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
INF = np.float32(np.inf)
KS = (1, 2, 5, 16)


def truncate(ref, K):
    """brute32_k(..., K) from the rows of a larger K"""
    return np.ascontiguousarray(ref[0][:, :K]), ref[1]


def mixed_points(sc, seed, n=130, n_feature=40):
    """near the surface, in the volume, 50 diagonals away, on vertices and edges: 3 n + 3 n_feature points, r_max = inf"""
    return np.concatenate(list(point_sets(sc, n, seed).values()) + [feature_points(sc, n_feature, seed + 1)])


def gpu_k(ctx, pts, K, cull=0xFF, attributes=False, counts=True):
    import torch
    res = ctx.closest_point_device_hits(dev(pts), K, cull_mask=cull, attributes=attributes, counts=counts)
    torch.cuda.synchronize()
    return res.numpy()


def check_rows(got, ref, what=""):
    """the GPU's (rows, attributes, counts) against (rows, counts) of brute32_k, byte for byte"""
    h, _, c = got
    rh, rc = ref
    if h is not None and h.tobytes() != rh.tobytes():
        bad = np.nonzero((h.view(np.uint8).reshape(len(h), -1) != rh.view(np.uint8).reshape(len(h), -1)).any(axis=1))[0]
        raise AssertionError("%s: %d rows differ from the brute force, first point %d: gpu %s reference %s (count %d)" %
                             (what, len(bad), bad[0], h[bad[0]], rh[bad[0]], rc[bad[0]]))
    if c is not None:
        assert np.array_equal(c, rc), (what, np.nonzero(c != rc)[0][:5])


def check_both_walks(ctx, pts, ref, K, cull=0xFF, what=""):
    """the counting walk (bounded by the radius alone) and the pruning walk (no counts): the reference's rows from both"""
    check_rows(gpu_k(ctx, pts, K, cull), truncate(ref, K), "%s, K %d with counts" % (what, K))
    h, _, c = gpu_k(ctx, pts, K, cull, counts=False)
    assert c is None
    check_rows((h, None, None), truncate(ref, K), "%s, K %d pruned" % (what, K))


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_exports_abi_and_null_context():
    assert "rt_closest_point_device_hits" in api.EXPORTS and "rt_closest_point_hits" in api.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^int rt_closest_point_device_hits\(rt_ctx\* ctx, size_t n, const void\* d_points4, uint32_t cull_mask, uint32_t max_hits,\s+"
                     r"void\* d_hits, void\* d_attr, void\* d_counts, void\* hip_stream\);", hdr, re.M)
    assert re.search(r"^int rt_closest_point_hits\(rt_ctx\* ctx, size_t n, const float\* points4_host, uint32_t cull_mask, uint32_t max_hits,\s+"
                     r"rt_hit\* hits_host, uint32_t\* counts_host, int counting, rt_stats\* stats\);", hdr, re.M)
    L = api.lib()
    assert hasattr(L, "rt_closest_point_device_hits") and hasattr(L, "rt_closest_point_hits") and L.rt_abi_version() == 7
    assert L.rt_closest_point_device_hits(None, 0, None, 0xFF, 1, None, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_closest_point_device_hits(None, 64, None, 0xFF, 4, None, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_closest_point_hits(None, 0, None, 0xFF, 1, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert hasattr(RtContext, "closest_point_device_hits") and hasattr(RtContext, "closest_point_hits")


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_the_walk_kernels_keep_the_record_level_budget(target):
    """k_closest_hits and its counting form: no scratch, no spills, the 12 KB stack in LDS, 4 waves per SIMD or more; the side kernel of
    the rows uses no scratch and spills nothing; one of each in both libraries"""
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    walk = [(n, r) for n, r in kernels.items() if re.search(r"k_closest_hits(_count)?E", n)]
    side = [(n, r) for n, r in kernels.items() if "k_closest_hits_side" in n]
    assert len(walk) == 2 and len(side) == 1, "\n".join(kernels)
    assert sum("k_closest_hits_count" in n for n, _ in walk) == 1
    for name, r in walk:
        assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert int(r["Occupancy"]) >= 4 and int(r["LDS Size"]) == 12288, (name, r)
    for name, r in side:
        assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)


def test_reference_against_itself():
    """brute32_k's first entry is closest_reference.brute32 byte for byte; rows have non-decreasing t and distinct (inst, prim); the
    counts with r_max = inf are the admitted triangles whose d2 is not NaN; the row distances agree with the sorted binary64
    per-triangle distances within 1e-5 t + 1e-6 M"""
    verts, idx, ranges, inst = small_scene()
    sc = cr.Scene(verts, idx, ranges, inst)
    sets = point_sets(sc, 60, seed=31)
    sets["features"] = feature_points(sc, 20, seed=32)
    K = 6
    adm = np.nonzero(sc.admitted(0xFF))[0]                # (a record of mask 0 is no candidate)
    A, B, C = sc.A[adm][None], sc.B[adm][None], sc.C[adm][None]
    N = np.cross(B - A, C - A)
    nn = (N * N).sum(-1)
    tri_mag = np.maximum(np.maximum(np.abs(sc.A).max(-1), np.abs(sc.B).max(-1)), np.abs(sc.C).max(-1))
    assert 0 < len(adm) < sc.n_tris
    for name, pts in sets.items():
        for cull in (0xFF, 0x5A):
            one, c1 = chr_.brute32_k(sc, pts, 1, cull)
            assert one[:, 0].tobytes() == cr.brute32(sc, pts, cull).tobytes(), (name, cull)
            rows, counts = chr_.brute32_k(sc, pts, K, cull)
            assert np.array_equal(c1, counts) and rows[:, :1].tobytes() == one.tobytes()
            assert (np.diff(rows["t"], axis=1) >= 0).all(), name
            ids = rows["inst"].astype(np.int64) * 1000 + rows["prim"]
            assert all(len(set(r)) == K for r in ids), name
            _, d2, _, _ = chr_.all_d2(sc, pts, cull)
            assert np.array_equal(counts, (~np.isnan(d2)).sum(axis=1))
        rows, _ = chr_.brute32_k(sc, pts, K)
        d64, _, _ = cr._tri_d2_64(pts[:, None, :3].astype(np.float64), A, B, C, N, nn)
        order = np.argsort(d64, axis=1)[:, :K]
        t64 = np.sqrt(np.take_along_axis(d64, order, axis=1))
        first = np.concatenate([[0], np.cumsum(np.bincount(sc.inst, minlength=len(sc.mask)))])
        mag = np.maximum(np.abs(pts[:, :3]).max(-1)[:, None], np.maximum(tri_mag[adm[order]], tri_mag[first[rows["inst"]] + rows["prim"]]))
        err, tol = np.abs(rows["t"].astype(np.float64) - t64), cr.t_tolerance(t64, mag)
        print("%s: worst row distance error %.3g of its bound" % (name, (err / tol).max()))
        assert (err <= tol).all(), (name, (err / tol).max())
    # radii, invalid records, count only
    pts = sets["volume"]
    full = chr_.brute32_k(sc, pts, K)
    q = pts.copy(); q[:, 3] = full[0]["t"][:, 2] * np.float32(1.0001)
    rows, counts = chr_.brute32_k(sc, q, K)
    assert (counts >= 3).all() and (counts < K).any() and (rows["inst"][np.arange(len(q)), np.minimum(counts, K - 1)] == -1)[counts < K].all()
    assert np.array_equal(rows["t"][counts < K, K - 1], q[counts < K, 3])
    bad = invalid_records(pts)
    rows, counts = chr_.brute32_k(sc, bad, 3)
    assert (counts[:6] == 0).all() and (rows["inst"][:6] == -1).all()
    assert np.array_equal(rows["t"][:7].view(np.uint32), np.repeat(bad[:7, 3:4], 3, axis=1).view(np.uint32))
    rows, counts = chr_.brute32_k(sc, pts, 0)
    assert rows.shape == (len(pts), 0) and np.array_equal(counts, full[1])


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def small():
    """small_scene, its numpy scene and oracle, about 500 mixed points and their 16 nearest triangles"""
    verts, idx, ranges, inst = small_scene(seed=51)
    sc = cr.Scene(verts, idx, ranges, inst)
    pts = mixed_points(sc, seed=52)
    assert len(pts) % 64 != 0
    return dict(geom=(verts, idx, ranges, inst), sc=sc, orc=oracle_scene(verts, idx, ranges, inst), pts=pts, ref=chr_.brute32_k(sc, pts, 16))


def load_small(ctx, small):
    verts, idx, ranges, inst = small["geom"]
    ctx.upload_geometry(verts, idx, ranges)
    ctx.set_instances(inst)


@pytest.mark.gpu
def test_rows_and_counts(ctx, small):
    """K 1, 2, 5 and 16 with counts and without: the same rows, the reference's; entry 0 is rt_closest_point_device's record; counts;
    count only; with r_max = inf the count is every admitted triangle whose d2 is not NaN"""
    import torch
    load_small(ctx, small)
    sc, pts, ref = small["sc"], small["pts"], small["ref"]
    single = ctx.closest_point_device(dev(pts))
    torch.cuda.synchronize()
    single = single.numpy()[0]
    assert single.tobytes() == cr.brute32(sc, pts).tobytes()
    for K in KS:
        check_both_walks(ctx, pts, ref, K, what="small scene")
        for counts in (True, False):
            h, _, _ = gpu_k(ctx, pts, K, counts=counts)
            assert np.ascontiguousarray(h[:, 0]).tobytes() == single.tobytes(), (K, counts)
    h, a, c = gpu_k(ctx, pts, 0)
    assert h is None and a is None and np.array_equal(c, ref[1])
    _, d2, _, _ = chr_.all_d2(sc, pts)
    assert np.array_equal(c, (~np.isnan(d2)).sum(axis=1)) and (c > 16).all()


@pytest.mark.gpu
def test_radius_classes_around_k(ctx, small):
    """radii midway between consecutive distances of the reference's rows: |C| of 0, 1, K - 1, K, K + 1 and more; and the inclusive
    bound on a constructed case, r_max * r_max == d2 exactly"""
    load_small(ctx, small)
    sc, pts, ref = small["sc"], small["pts"][:390], small["ref"]          # (without the feature points: their first distances are 0)
    t = ref[0]["t"][:390].astype(np.float64)
    K = 4
    want = np.array([0, 1, K - 1, K, K + 1, 9])[np.arange(len(pts)) % 6]
    lo = np.where(want > 0, t[np.arange(len(pts)), np.maximum(want - 1, 0)], 0.0)
    hi = t[np.arange(len(pts)), want]
    q = pts.copy(); q[:, 3] = ((lo + hi) / 2).astype(np.float32)
    rq = chr_.brute32_k(sc, q, 16)
    # (triangles at equal distances, around a vertex or an edge, enter together: such a point lands in a neighbouring class)
    assert (rq[1] == want).mean() > 0.8 and all((rq[1] == w).sum() > 30 for w in np.unique(want))
    for k in (K, 1, 16):
        check_both_walks(ctx, q, rq, k, what="radius classes")
    check_rows(gpu_k(ctx, q, 0), (None, rq[1]), "radius classes, count only")
    # d2 == r_max * r_max exactly: the point 2 above the interior of an integer triangle; a second one 2 + 2^-22 away
    z = -np.float32(2.0) ** -22
    pos = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, z], [4, 0, z], [0, 4, z]], np.float32)
    verts = np.concatenate([pos, np.tile([[0, 0, 1]], (6, 1))], axis=1).astype(np.float32).reshape(-1)
    idx, ranges = np.arange(6, dtype=np.uint32), [(0, 0, 2)]
    inst = np.asarray([host.make_instance(irc.IDENTITY, 0, 0)], INSTANCE_DTYPE)
    sc2, _ = load(ctx, verts, idx, ranges, inst)
    p = np.array([[1, 1, 2, 2], [1, 1, 2, np.nextafter(np.float32(2), INF)], [1, 1, 2, np.nextafter(np.float32(2), np.float32(0))]], np.float32)
    r2 = chr_.brute32_k(sc2, p, 2)
    assert list(r2[1]) == [1, 2, 0] and r2[0][0, 0]["prim"] == 0 and r2[0][0, 0]["t"] == 2 and r2[0][0, 1]["prim"] == -1
    for k in (1, 2):
        check_both_walks(ctx, p, r2, k, what="inclusive radius")
    check_rows(gpu_k(ctx, p, 0), (None, r2[1]), "inclusive radius, count only")


def tie_scene(seed=71):
    """small_scene's first twelve records and copies of four of them (identical transform and mesh: every d2 ties across inst), every
    record visible; `moved`: the same records displaced, the copies with their originals"""
    verts, idx, ranges, inst = small_scene(seed=seed, n=12)
    inst["custom_index_and_mask"] |= np.uint32(0xFF000000)
    rng = np.random.default_rng(seed + 1)
    moved = inst.copy()
    moved["transform"][:, [3, 7, 11]] += rng.uniform(-0.3, 0.3, (len(inst), 3)).astype(np.float32)
    twice = lambda r: np.concatenate([r, r[[1, 4, 6, 7]]])   # noqa: E731
    return verts, idx, ranges, twice(inst), twice(moved)


_TIES = {}


def tie_cases():
    """(points, {records name: (numpy scene, reference rows of 16)}), computed once: near points and points exactly on shared vertices"""
    if not _TIES:
        verts, idx, ranges, inst, moved = tie_scene()
        sc = cr.Scene(verts, idx, ranges, inst)
        pts = np.concatenate([point_sets(sc, 50, seed=73)["near"], feature_points(sc, 43, seed=74)])
        assert len(pts) % 64 != 0
        _TIES["x"] = (pts, {"placed": (sc, chr_.brute32_k(sc, pts, 16)),
                            "moved": (cr.Scene(verts, idx, ranges, moved), chr_.brute32_k(cr.Scene(verts, idx, ranges, moved), pts, 16))})
    return _TIES["x"]


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "1", "2", "3"])
def test_ties_under_every_tree(builder, monkeypatch):
    """d2 ties across inst (identical records) and across prim (points on shared vertices), the K-th and (K + 1)-th candidates among
    them: the smaller (inst, prim) stays, under every BLAS builder, host and device instance records and their refits"""
    import torch
    verts, idx, ranges, inst, moved = tie_scene()
    pts, cases = tie_cases()
    sc, ref = cases["placed"]
    _, d2, _, _ = chr_.all_d2(sc, pts)
    s = np.sort(d2, axis=1)
    for K in (1, 3, 5):      # the premise: the K-th and (K + 1)-th smallest d2 tie for many points
        assert (s[:, K - 1] == s[:, K]).sum() > 20, K
    assert ((ref[0]["t"][:, 0] == ref[0]["t"][:, 1]) & (ref[0]["inst"][:, 0] != ref[0]["inst"][:, 1])).sum() > 10     # across inst
    assert ((ref[0]["t"][:, 0] == ref[0]["t"][:, 1]) & (ref[0]["inst"][:, 0] == ref[0]["inst"][:, 1])).sum() > 5      # across prim
    c = RtContext(0)
    try:
        use_builder(c, builder, monkeypatch)
        c.upload_geometry(verts, idx, ranges)
        for source in ("host", "device"):
            for name, records, update in (("placed", inst, False), ("moved", moved, True)):
                if source == "host":
                    c.set_instances(records, update=update)
                else:
                    torch.cuda.synchronize()
                    c.set_instances_device(dev_inst(records), update=update)
                for K in (1, 3, 5, 16):
                    check_both_walks(c, pts, cases[name][1], K, what="%s records %s, update %d, builder %s" % (source, name, update, builder))
    finally:
        c.close()


@pytest.mark.gpu
def test_cull_masks_and_bad_instance_records(ctx, small):
    """every single-bit cull mask and 0xFF; a void record is never a candidate, a non-invertible one answers over its o2w image"""
    verts, idx, ranges, inst = small["geom"]
    bad = inst.copy()
    bad[5] = irc.VOID["tr_pinf"][0](bad[5])
    bad[9] = irc.NONINVERTIBLE["rank2"][0](bad[9])
    ctx.upload_geometry(verts, idx, ranges)
    ctx.set_instances(bad)
    with np.errstate(all="ignore"):
        sc = cr.Scene(verts, idx, ranges, irc.twin_records(bad, [5]))    # (the void record: mask 0; the non-invertible one as it is)
    pts = small["pts"][::2].copy()
    pts[1::3, 3] = 2.5
    assert len(pts) % 64 != 0
    seen = 0
    for cull in [1 << b for b in range(8)] + [0xFF]:
        ref = chr_.brute32_k(sc, pts, 5, cull)
        check_both_walks(ctx, pts, ref, 5, cull, what="cull %#x" % cull)
        check_rows(gpu_k(ctx, pts, 0, cull), (None, ref[1]), "cull %#x, count only" % cull)
        assert not (ref[0]["inst"] == 5).any()
        assert ((sc.mask[ref[0]["inst"][ref[0]["inst"] >= 0]] & cull) != 0).all()
        seen += (ref[0]["inst"] == 9).sum()
    assert seen > 0, "the non-invertible record's image is among the nearest triangles of some points"


@pytest.mark.gpu
def test_invalid_point_records(ctx, small):
    """NaN / inf coordinates, negative and NaN radii: miss rows that keep r_max's bit pattern (NaN, -0.0), a count of 0"""
    load_small(ctx, small)
    bad = invalid_records(small["pts"][130:260])
    ref = chr_.brute32_k(small["sc"], bad, 3)
    got = gpu_k(ctx, bad, 3)
    check_rows(got, ref, "invalid records")
    check_both_walks(ctx, bad, ref, 3, what="invalid records")
    assert (got[2][:6] == 0).all() and (got[0]["inst"][:7] == -1).all()
    assert np.array_equal(got[0]["t"][:7].view(np.uint32), np.repeat(bad[:7, 3:4], 3, axis=1).view(np.uint32))
    check_rows(gpu_k(ctx, bad, 0), (None, ref[1]), "invalid records, count only")


def nan_soup(seed):
    """degenerate_soup (needles, zero-area triangles) and twelve triangles whose first two vertices coincide: for a point on the third
    vertex's side the edge-AB region divides 0 by 0 and d2 is NaN"""
    verts, idx, ranges = degenerate_soup(seed)
    rng = np.random.default_rng(seed + 100)
    a = rng.uniform(-1, 1, (12, 3))
    pos = np.stack([a, a, a + rng.uniform(-0.5, 0.5, (12, 3))], axis=1).reshape(-1, 3)
    extra = np.concatenate([pos, np.tile([[0, 0, 1]], (len(pos), 1))], axis=1).astype(np.float32).reshape(-1)
    n = len(idx)
    return np.concatenate([verts, extra]), np.concatenate([idx, np.arange(n, n + 36, dtype=np.uint32)]), [(0, 0, n // 3 + 12)]


@pytest.mark.gpu
def test_degenerate_and_far_geometry(ctx):
    """zero-area triangles and needles: a NaN d2 is never listed or counted; the scene 1e4 from the origin: the translation's slack"""
    verts, idx, ranges = nan_soup(62)
    inst = placed_instances(12, 63, spacing=2.5, n_meshes=1)
    sc, _ = load(ctx, verts, idx, ranges, inst)
    pts = mixed_points(sc, seed=64, n=60, n_feature=30)
    ref = chr_.brute32_k(sc, pts, 16)
    _, d2, _, _ = chr_.all_d2(sc, pts)
    nan = np.isnan(d2)
    print("degenerate soup: %d of %d d2 are NaN" % (nan.sum(), d2.size))
    assert nan.any(axis=1).mean() > 0.9 and np.array_equal(ref[1], (~nan).sum(axis=1)) and (ref[1] > 16).all()
    for K in (1, 4, 16):
        check_both_walks(ctx, pts, ref, K, what="degenerate soup")
        assert not np.isnan(gpu_k(ctx, pts, K)[0]["t"]).any()
    verts, idx, ranges, inst = small_scene(seed=81, offset=1e4)
    sc, _ = load(ctx, verts, idx, ranges, inst)
    pts = mixed_points(sc, seed=82, n=60, n_feature=30)
    ref = chr_.brute32_k(sc, pts, 16)
    q = pts.copy(); q[:, 3] = ref[0]["t"][:, 5] * np.float32(1.25)
    rq = chr_.brute32_k(sc, q, 16)
    for K in (1, 4, 16):
        check_both_walks(ctx, pts, ref, K, what="offset 1e4")
        check_both_walks(ctx, q, rq, K, what="offset 1e4, radii")


@pytest.mark.gpu
def test_attributes(ctx, small):
    """P, N and objectIndex against the oracle's hit_attributes of the returned records, side words with point i // K; misses are
    zeros, -1 and 0"""
    load_small(ctx, small)
    sc, orc = small["sc"], small["orc"]
    pts = small["pts"].copy()
    pts[::3, 3] = small["ref"][0]["t"][::3, 2] * np.float32(1.001)      # (rows that end in misses)
    K = 5
    ref = chr_.brute32_k(sc, pts, K)
    assert (ref[1] < K).sum() > 50
    for counts in (True, False):
        h, a, c = gpu_k(ctx, pts, K, attributes=True, counts=counts)
        check_rows((h, a, c), ref, "attributes")
        assert a.shape == (len(pts), K, 8)
        flat, recs = a.reshape(-1, 8), np.ascontiguousarray(h.reshape(-1))
        kinds, _ = cr.side_words(sc, np.repeat(pts, K, axis=0), recs)
        assert np.array_equal(flat[:, 7].view(np.uint32), kinds)
        assert set(np.unique(kinds)) == {0, cr.FRONT, cr.BACK}
        o = orc.hit_attributes(recs)
        f = flat.view(np.float32)
        assert np.array_equal(f[:, 0:3].view(np.uint32), o[:, 0:3].view(np.uint32))
        assert np.array_equal(f[:, 4:7].view(np.uint32), o[:, 3:6].view(np.uint32))
        assert np.array_equal(flat[:, 3], o[:, 6].astype(np.int32))
        miss = recs["inst"] < 0
        assert miss.any() and (flat[miss, 0:3] == 0).all() and (flat[miss, 4:7] == 0).all() and (flat[miss, 7] == 0).all() and (flat[miss, 3] == -1).all()


@pytest.mark.gpu
def test_the_spill_half_of_the_stack(corridors):
    """the corridor world of tests/test_stack_spill.py.  With counts the walk is bounded by the radius alone, which is the walk the CPU
    stack model walks: the deep targets reach STACK2_LDS + 2 entries, the shallow ones stay in LDS.  Without counts (K = 4) pruning
    shortens the walk: the reference only."""
    w = corridors
    pts, tag, single = closest_points_and_reference(w)
    closest_premise(w, pts, tag)
    ref = chr_.brute32_k(w.sc, pts, 16)
    assert ref[0][:, 0].tobytes() == single.tobytes() and ref[1].max() == w.sc.n_tris
    for K, counts in ((16, True), (1, True), (4, False)):
        h, _, c = gpu_k(w.ctx, pts, K, counts=counts)
        check_rows((h, None, c), truncate(ref, K), "corridors, K %d, counts %s" % (K, counts))
        assert (c is None) == (not counts)


@pytest.mark.gpu
def test_more_points_than_the_resident_grid_has_threads(ctx, small):
    """valid, invalid and far points interleaved (lanes refill in the middle of a wave), repeated until there are more of them than
    the resident grid has threads: every wave takes several chunks"""
    load_small(ctx, small)
    sc = small["sc"]
    sets = point_sets(sc, 130, seed=91)
    near = sets["near"].copy(); near[::2, 3] = chr_.brute32_k(sc, near[::2], 2)[0]["t"][:, 1] * np.float32(1.0001)      # (two candidates or a few more)
    parts = [near, np.tile(invalid_records(sets["volume"]), (11, 1))[:130], sets["far"], sets["volume"]]
    pts = np.stack(parts, axis=1).reshape(-1, 4)
    K = 4
    ref = chr_.brute32_k(sc, pts, K)
    assert (ref[1] == 0).sum() > 60 and (ref[1] == ref[1].max()).sum() > 200 and ((ref[1] > 0) & (ref[1] < K)).any()
    reps = 256 * 8 * 256 // len(pts) + 2
    many = np.tile(pts, (reps, 1))
    assert len(many) > 256 * 8 * 256 and len(many) % 64 != 0       # (MI355X: 256 CUs, at most 8 resident workgroups of 256 threads each)
    want = np.tile(ref[0], (reps, 1)).tobytes()
    for counts in (True, False):
        h, _, c = gpu_k(ctx, many, K, counts=counts)
        assert h.tobytes() == want, counts
        assert c is None if not counts else np.array_equal(c, np.tile(ref[1], reps))


# ---- plumbing -----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_host_form_counting_and_stream_order(ctx, small):
    """the host form equals the device form; counting fills both counters, and for K = 1 without counts they equal rt_closest_point's
    on the same points (the same pruning); out= reuse; a query on a side stream behind a kernel that writes its points; n == 0"""
    import torch
    load_small(ctx, small)
    pts, ref = small["pts"], small["ref"]
    K = 5
    for counts in (True, False):
        h, c, st = ctx.closest_point_hits(pts, K, counts=counts)
        check_rows((h, None, c), truncate(ref, K), "host form")
        assert (c is None) == (not counts) and st.node_visits == 0 and st.tri_tests == 0 and st.bvh_node_bytes == 32 and st.bvh_tri_bytes == 48
    h, c, st = ctx.closest_point_hits(pts, 0)
    assert h is None and np.array_equal(c, ref[1])
    h, c, st = ctx.closest_point_hits(pts, K, counting=True)
    check_rows((h, None, c), truncate(ref, K), "host form, counting")
    assert st.node_visits > 0 and st.tri_tests == int(ref[1].sum()) and st.ms_trace_closest > 0
    _, st1 = ctx.closest_point(pts, counting=True)
    h, c, stk = ctx.closest_point_hits(pts, 1, counts=False, counting=True)
    assert c is None and h.tobytes() == truncate(ref, 1)[0].tobytes()
    assert (stk.node_visits, stk.tri_tests) == (st1.node_visits, st1.tri_tests) and 0 < stk.tri_tests < st.tri_tests
    assert ctx.closest_point_hits(pts, 2, cull_mask=0)[0]["inst"].max() == -1
    # out= reuse
    src = dev(pts)
    n = len(pts)
    bufs = (torch.empty((n, K, 5), dtype=torch.int32, device="cuda:0"), torch.empty((n, K, 8), dtype=torch.int32, device="cuda:0"),
            torch.empty((n,), dtype=torch.int32, device="cuda:0"))
    res = ctx.closest_point_device_hits(src, K, attributes=True, out=bufs)
    assert res.hits.data_ptr() == bufs[0].data_ptr() and res.attr.data_ptr() == bufs[1].data_ptr() and res.count.data_ptr() == bufs[2].data_ptr()
    check_rows(res.numpy(), truncate(ref, K), "out=")
    with pytest.raises(ValueError):
        ctx.closest_point_device_hits(src, K, out=(bufs[0][:-1], None, bufs[2]))
    # stream order
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = slow_queue(torch, 12)
        p = (src + (a[0, 0] != a[0, 0]).to(torch.float32) * 0).contiguous()   # made behind the queue, on s
        r1 = ctx.closest_point_device_hits(p, K, attributes=True, stream=s)
        r2 = ctx.closest_point_device(p, stream=s)
        r3 = ctx.closest_point_device_hits(p, 2, counts=False, stream=s)
        p.zero_()                                                             # overwritten right after the calls
        h1, c1, h2, h3 = r1.hits.clone(), r1.count.clone(), r2.hits.clone(), r3.hits.clone()
    s.synchronize()
    assert h1.cpu().numpy().view(HIT_DTYPE).reshape(n, K).tobytes() == truncate(ref, K)[0].tobytes()
    assert np.array_equal(c1.cpu().numpy().view(np.uint32), ref[1])
    assert h2.cpu().numpy().view(HIT_DTYPE).reshape(-1).tobytes() == truncate(ref, 1)[0].tobytes()
    assert h3.cpu().numpy().view(HIT_DTYPE).reshape(n, 2).tobytes() == truncate(ref, 2)[0].tobytes()
    # n == 0
    e = ctx.closest_point_device_hits(torch.empty((0, 4), dtype=torch.float32, device="cuda:0"), 3, attributes=True)
    assert e.hits.shape == (0, 3, 5) and e.attr.shape == (0, 3, 8) and e.count.shape == (0,)
    h, c, _ = ctx.closest_point_hits(np.zeros((0, 4), np.float32), 3)
    assert h.shape == (0, 3) and len(c) == 0


def _raw(c, n, pts, cull, k, hits, attr, counts):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_closest_point_device_hits(c.h, n, p(pts), cull, k, p(hits), p(attr), p(counts), None)


@pytest.mark.gpu
def test_error_statuses():
    import torch
    from tests.test_blas_refit import span
    sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
    sc = cr.Scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances)
    pts_np = point_sets(sc, 100, seed=121)["near"]
    pts_np[:, 3] = 0.05
    K = 4
    ref = chr_.brute32_k(sc, pts_np, K)
    pts = dev(pts_np)
    n = pts.shape[0]
    hits = torch.empty((n + 1, K, 5), dtype=torch.int32, device="cuda:0")
    attr = torch.empty((n + 1, K, 8), dtype=torch.int32, device="cuda:0")
    cnt = torch.empty((n + 1,), dtype=torch.int32, device="cuda:0")
    P_, H_, A_, C_ = pts.data_ptr(), hits.data_ptr(), attr.data_ptr(), cnt.data_ptr()
    c = RtContext(0)

    def err(args, code, text):
        assert _raw(c, *args) == code, args
        msg = c.L.rt_last_error(c.h).decode()
        assert text in msg, (args, msg)

    def ok():
        res = c.closest_point_device_hits(pts, K)
        torch.cuda.synchronize()
        check_rows(res.numpy(), ref, "after an error")

    good = (n, P_, 0xFF, K, H_, 0, C_)
    try:
        err(good, RT_ERR_NOT_READY, "")   # no geometry
        c.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        err(good, RT_ERR_NOT_READY, "")   # no TLAS
        c.set_instances(sp.instances)
        c.set_uniforms(sp.uniforms)
        ok()
        bad = [((0xFFFFFF00, P_, 0xFF, K, H_, 0, C_), "too many points"), ((0x40000000, P_, 0xFF, K, H_, 0, C_), "n * max_hits"),
               ((n, P_, 0xFF, 17, H_, 0, C_), "max_hits must be 0..16"), ((n, P_, 0x100, K, H_, 0, C_), "cull_mask"),
               ((n, P_, 0xFF, 0, H_, 0, C_), "counts only"), ((n, P_, 0xFF, 0, 0, A_, C_), "counts only"), ((n, P_, 0xFF, 0, 0, 0, 0), "counts only"),
               ((n, 0, 0xFF, K, H_, 0, C_), "null point/hit pointers"), ((n, P_, 0xFF, K, 0, 0, C_), "null point/hit pointers"),
               ((n, P_ + 4, 0xFF, K, H_, 0, C_), "aligned"), ((n, P_, 0xFF, K, H_ + 2, 0, C_), "aligned"), ((n, P_, 0xFF, K, H_, A_ + 4, C_), "aligned"),
               ((n, P_, 0xFF, K, H_, 0, C_ + 2), "aligned")]
        host_buf = np.zeros((n + 1, K, 8), np.float32)
        pinned = torch.zeros((n, K, 8), dtype=torch.float32).pin_memory()
        for ptr in ((host_buf.ctypes.data + 15) & ~15, pinned.data_ptr()):   # (16-byte aligned: only the memory kind is wrong)
            bad += [((n, ptr, 0xFF, K, H_, 0, C_), "device memory of the context's GPU"), ((n, P_, 0xFF, K, ptr, 0, C_), "device memory of the context's GPU"),
                    ((n, P_, 0xFF, K, H_, ptr, C_), "device memory of the context's GPU"), ((n, P_, 0xFF, K, H_, 0, ptr), "device memory of the context's GPU")]
        for args, text in bad:
            err(args, RT_ERR_INVALID_ARGUMENT, text)
        ok()
        assert _raw(c, n, P_, 0xFF, K, H_, 0, 0) == 0 and _raw(c, n, P_, 0xFF, 0, 0, 0, C_) == 0      # no counts; counts only
        torch.cuda.synchronize()
        assert np.array_equal(cnt[:n].cpu().numpy().view(np.uint32), ref[1])
        out, oc = np.zeros((n, K), HIT_DTYPE), np.zeros(n, np.uint32)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        host_form = c.L.rt_closest_point_hits
        assert host_form(c.h, n, None, 0xFF, K, vp(out), vp(oc), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert host_form(c.h, n, vp(pts_np), 0xFF, K, None, vp(oc), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert host_form(c.h, n, vp(pts_np), 0x100, K, vp(out), vp(oc), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert host_form(c.h, n, vp(pts_np), 0xFF, 17, vp(out), vp(oc), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert host_form(c.h, n, vp(pts_np), 0xFF, 0, vp(out), vp(oc), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert host_form(c.h, n, vp(pts_np), 0xFF, 0, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert host_form(c.h, n, vp(pts_np), 0xFF, K, vp(out), None, 0, None) == 0 and out.tobytes() == ref[0].tobytes()
        assert _raw(c, 0, 0, 0xFF, K, 0, 0, 0) == 0   # n == 0 enqueues nothing and needs no pointers
        with pytest.raises(ValueError):
            c.closest_point_device_hits(pts.cpu(), K)
        with pytest.raises(ValueError):
            c.closest_point_device_hits(torch.zeros((4, 8), dtype=torch.float32, device="cuda:0"), K)
        with pytest.raises(ValueError):
            c.closest_point_device_hits(pts, 17)
        with pytest.raises(ValueError):
            c.closest_point_device_hits(pts, 0, counts=False)
        with pytest.raises(RtError) as e:
            c.closest_point_device_hits(pts, K, cull_mask=0x1FF)
        assert e.value.code == RT_ERR_INVALID_ARGUMENT
        ok()
        # not ready: a stale TLAS after a BLAS refit, then a frame batch
        ff, nf = span(sp.geom, 1)
        v = torch.from_numpy(sp.geom.verts[ff:ff + nf].copy()).to("cuda:0")
        torch.cuda.synchronize()
        c.refit_blas_device(1, v)
        err(good, RT_ERR_NOT_READY, "")
        c.set_instances(sp.instances)
        ok()
        c.set_batch(np.stack([sp.instances, sp.instances]), np.stack([sp.uniforms, sp.uniforms]).reshape(-1))
        err(good, RT_ERR_NOT_READY, "")
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
        err(good, RT_ERR_INVALID_ARGUMENT, "trace_variant 0")
        a.set_param("trace_variant", 0)
        a.set_instances(sp.instances)
        ok()
    finally:
        a.close()
