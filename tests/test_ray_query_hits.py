"""rt_intersect_device_hits: every candidate along a ray (rayQueryProceedEXT's loop in data form), the first K of them in (t, inst, prim)
order and how many there are.

The expected lists come from the oracle alone: orc_query_candidate decides, bit for bit, whether a ray accepts an (instance, primitive) and
with which t, u, v and hit kind; running it over every triangle of the scene and sorting gives the exact list (oracle_lists).  The CPU part
checks that helper against orc_intersect_query (entry 0 is the closest hit) and against the binary64 brute force of tests/query_reference.py
(the counts); the GPU part holds the library to it byte for byte: every valid call flag value, per-ray words, K from 1 to 16 with and
without counts (the pruned walk), attributes and hit kinds, equal-t geometry, count-only calls, a 1 M-ray batch on the cfg3 scene, inside /
outside parity, every instance-record source and BLAS writer, stream order, frames in flight beside a query, and the error statuses."""
import ctypes
import os
import types

import numpy as np
import pytest

from tests import query_reference as ref64
from tests import scenes
from tests.test_ray_query import PATHS, dev, dev_inst, edge_rays, mixed_rays, slow_queue
from tests.test_ray_query_oracle import (CULL_BACK, CULL_FRONT, CULL_NO_OPAQUE, NO_OPAQUE, OPAQUE, SKIP_AABBS, TERMINATE, aimed_rays, edge_geometry,
                                         edge_geometry_rays, edge_instances, grazing, oracle_scene, placed_instances, random_words, small_meshes,
                                         use_builder, valid_call_flags)
from vulkan_raytracing_amd import RtContext, api, host, workloads
from vulkan_raytracing_amd.api import HIT_DTYPE, RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
KS = (1, 2, 3, 8, 16)


# ---- the exact expected lists -------------------------------------------------------------------------------------------------

def hits_scene(verts, idx, ranges, inst):
    """oracle_scene, with the triangle count of every instance (what oracle_lists walks over)"""
    orc = oracle_scene(verts, idx, ranges, inst)
    orc.tri_counts = np.array([ranges[int(r["mesh"])][2] for r in inst], np.int64)
    return orc


def oracle_lists(orc, rays, words, flags, cull, K, chunk=1 << 20):
    """OracleScene.query_candidate over every (inst, prim) of the scene for every ray: the accepted candidates sorted by (t, inst, prim),
    the first K of them per ray with rt_intersect's miss after them -> (HIT_DTYPE (n, K), uint32 kinds (n, K), uint32 counts (n,))"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    n = len(rays)
    w = np.full(n, 0xFF000000, np.uint32) if words is None else np.asarray(words, np.uint32)
    tc = orc.tri_counts
    inst_ids = np.repeat(np.arange(len(tc), dtype=np.int32), tc)
    prim_ids = np.concatenate([np.arange(c, dtype=np.int32) for c in tc])
    T = len(inst_ids)
    per = max(1, chunk // T)
    parts = []
    for r0 in range(0, n, per):
        r1 = min(n, r0 + per)
        ri = np.repeat(np.arange(r0, r1), T)
        ok, c, k = orc.query_candidate(rays[ri], np.tile(inst_ids, r1 - r0), np.tile(prim_ids, r1 - r0), w[ri], flags, cull)
        parts.append((ri[ok], c[ok], k[ok]))
    ray = np.concatenate([p[0] for p in parts])
    c = np.concatenate([p[1] for p in parts])
    k = np.concatenate([p[2] for p in parts])
    order = np.lexsort((c["prim"], c["inst"], c["t"], ray))
    ray, c, k = ray[order], c[order], k[order]
    counts = np.bincount(ray, minlength=n)
    start = np.concatenate([[0], np.cumsum(counts)])[ray]
    pos = np.arange(len(ray)) - start
    sel = pos < K
    hits = np.zeros((n, K), HIT_DTYPE)
    hits["t"] = rays[:, 7][:, None]
    hits["prim"] = -1
    hits["inst"] = -1
    kinds = np.zeros((n, K), np.uint32)
    hits[ray[sel], pos[sel]] = c[sel]
    kinds[ray[sel], pos[sel]] = k[sel]
    return hits, kinds, counts.astype(np.uint32)


def truncate(ref, K):
    """oracle_lists(..., K) from the lists of a larger K"""
    return ref[0][:, :K].copy(), ref[1][:, :K].copy(), ref[2]


def small_scene(seed=5, n=32):
    """small_meshes (an octahedron, a soup of 12 triangles) under placed_instances: all 16 instance-flag combinations, eight masks"""
    verts, idx, ranges = small_meshes(seed)
    inst = placed_instances(n, seed + 1, spacing=3.0)
    return verts, idx, ranges, inst


def pool_rays(inst, verts, idx, ranges, n, seed):
    """aimed, grazing and far rays at the instances, mixed rays and the edge cases"""
    return np.concatenate([aimed_rays(inst, n, seed, radius=0.6), grazing(inst, verts, idx, ranges, max(n // 16, 8), seed + 1),
                           aimed_rays(inst, max(n // 8, 8), seed + 2, radius=0.6, far=True), mixed_rays(max(n // 16, 8), seed + 3), edge_rays()])


def gpu_hits(ctx, rays, words, flags, cull, K, attributes=False, counts=True):
    import torch
    w = None if words is None else torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32).copy()).to("cuda:0")
    res = ctx.intersect_device_hits(dev(rays), K, ray_flags=flags, cull_mask=cull, words=w, attributes=attributes, counts=counts)
    torch.cuda.synchronize()
    return res.numpy()


def check_lists(orc, got, ref, what=""):
    """the GPU's (hits, attributes, counts) against oracle_lists byte for byte; attributes against orc_hit_attributes and the oracle's
    kinds"""
    h, a, c = got
    rh, rk, rc = ref
    if h is not None and h.tobytes() != rh.tobytes():
        bad = np.nonzero((h.view(np.uint8).reshape(len(h), -1) != rh.view(np.uint8).reshape(len(h), -1)).any(axis=1))[0]
        raise AssertionError("%s: %d lists differ from the oracle, first ray %d: gpu %s oracle %s (count %d)" % (what, len(bad), bad[0], h[bad[0]], rh[bad[0]], rc[bad[0]]))
    if c is not None:
        assert np.array_equal(c, rc), (what, np.nonzero(c != rc)[0][:5])
    if a is not None:
        K = h.shape[1]
        flat = a.reshape(-1, 8)
        assert np.array_equal(flat[:, 7].view(np.uint32), rk.reshape(-1)), what
        o = orc.hit_attributes(np.ascontiguousarray(h.reshape(-1)))
        f = flat.view(np.float32)
        assert np.array_equal(f[:, 0:3].view(np.uint32), o[:, 0:3].view(np.uint32)), what
        assert np.array_equal(f[:, 4:7].view(np.uint32), o[:, 3:6].view(np.uint32)), what
        assert np.array_equal(flat[:, 3], o[:, 6].astype(np.int32)), what
        miss = h.reshape(-1)["inst"] < 0
        assert (flat[miss, 0:3] == 0).all() and (flat[miss, 4:7] == 0).all() and (flat[miss, 7] == 0).all(), what
        assert a.shape == (len(h), K, 8)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_export_abi_and_null_context():
    import re
    assert "rt_intersect_device_hits" in api.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^int rt_intersect_device_hits\(rt_ctx\* ctx, size_t n, const void\* d_rays8, const void\* d_ray_words, uint32_t ray_flags, uint32_t cull_mask,\s+"
                     r"uint32_t max_hits, void\* d_hits, void\* d_attr, void\* d_counts, void\* hip_stream\);", hdr, re.M)
    L = api.lib()
    assert hasattr(L, "rt_intersect_device_hits") and L.rt_abi_version() == 7
    assert L.rt_intersect_device_hits(None, 0, None, None, 0, 0xFF, 1, None, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_intersect_device_hits(None, 64, None, None, 0, 0xFF, 4, None, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert hasattr(RtContext, "intersect_device_hits")


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_hits_kernels_keep_the_record_level_budget(target):
    """the walk k_query_hits keeps the record-level walks' budget (>= 4 waves per SIMD, scratch <= 32 bytes, no spills); the attribute
    kernel k_query_hits_surface uses no scratch and spills nothing; one of each in both libraries"""
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    walk = [(n, r) for n, r in kernels.items() if "k_query_hits" in n and "k_query_hits_surface" not in n]
    surf = [(n, r) for n, r in kernels.items() if "k_query_hits_surface" in n]
    assert len(walk) == 1 and len(surf) == 1, "\n".join(kernels)
    for name, r in walk:
        assert int(r["Occupancy"]) >= 4 and int(r["ScratchSize"]) <= 32 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
    for name, r in surf:
        assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
    for name, _ in walk + surf:
        for taken in ("k_hit_attr", "k_hit_kind", "k_ray_ingest", "k_resolve_points", "k_packet", "k_trace", "k_blob", "k_tile", "k_beam_shadow"):
            assert taken not in name, name


def test_oracle_lists_check_themselves():
    """entry 0 is orc_intersect_query's closest hit bit for bit (TERMINATE stripped); the counts are the binary64 reference's surviving
    candidates on every ray it does not call ambiguous"""
    verts, idx, ranges, inst = small_scene()
    orc = hits_scene(verts, idx, ranges, inst)
    scene = ref64.Scene(verts, idx, ranges, inst)
    rays = pool_rays(inst, verts, idx, ranges, 2048, seed=301)
    words = random_words(len(rays), seed=302)
    total, multi = 0, 0
    for flags, cull in ((0, 0xFF), (CULL_BACK, 0xFF), (NO_OPAQUE, 0x5A), (CULL_FRONT | CULL_NO_OPAQUE, 0xA5)):
        h, k, c = oracle_lists(orc, rays, words, flags, cull, 4)
        closest, ck = orc.intersect_query(rays, words & ~np.uint32(TERMINATE), flags, cull)
        assert h[:, 0].tobytes() == closest.tobytes() and np.array_equal(k[:, 0], ck), (flags, cull)
        r = ref64.query(scene, rays, words, flags, cull)
        sure = ~r["ambiguous"]
        assert np.array_equal(c[sure], r["survivors"][sure].sum(axis=1)), (flags, cull)
        # the list itself: (t, inst, prim) strictly increasing, the misses after it
        n_in = np.minimum(c, 4)
        for j in range(3):
            both = n_in > j + 1
            a_, b_ = h[both, j], h[both, j + 1]
            assert ((a_["t"] < b_["t"]) | ((a_["t"] == b_["t"]) & ((a_["inst"] < b_["inst"]) | ((a_["inst"] == b_["inst"]) & (a_["prim"] < b_["prim"]))))).all()
        for j in range(4):
            m = n_in <= j
            assert (h[m, j]["inst"] == -1).all() and np.array_equal(h[m, j]["t"].view(np.uint32), rays[m, 7].view(np.uint32))
        total += sure.sum()
        multi += (c[sure] >= 2).sum()
    assert total > 0.9 * 4 * len(rays) and multi > 200, (total, multi)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_lists_every_call_flag_value(ctx):
    """every valid call flag value without TERMINATE, four cull masks in turn, K in turn over 1, 2, 3, 8, 16, with and without counts"""
    verts, idx, ranges, inst = small_scene(seed=311)
    ctx.upload_geometry(verts, idx, ranges)
    ctx.set_instances(inst)
    orc = hits_scene(verts, idx, ranges, inst)
    pool = pool_rays(inst, verts, idx, ranges, 8000, seed=312)
    pool = pool[np.random.default_rng(313).permutation(len(pool))]
    e = edge_rays()
    combos = [f for f in valid_call_flags() if not f & TERMINATE]
    assert len(combos) == 70
    full = 0
    for i, flags in enumerate(combos):
        cull = (0xFF, 0x01, 0x5A, 0x00)[i % 4]
        K = KS[i % len(KS)]
        k0 = (i * 397) % (len(pool) - 491)
        rays = np.concatenate([pool[k0:k0 + 491], e[i % 2::2][:9]])
        ref = oracle_lists(orc, rays, None, flags, cull, K)
        got = gpu_hits(ctx, rays, None, flags, cull, K, attributes=i % 3 == 0, counts=i % 2 == 0)
        check_lists(orc, got, ref, "flags %#x cull %#x K %d" % (flags, cull, K))
        full += (ref[2] > K).sum()
    assert full > 500, full   # rows cut at K: the pruned and the counting walk both meet them


@pytest.mark.gpu
def test_lists_per_ray_words(ctx):
    """per-ray words of every flag value (TERMINATE among them: ignored) and random cull masks, under call flags that combine with them;
    K over 1, 2, 3, 8, 16 with and without counts, with attributes"""
    verts, idx, ranges, inst = small_scene(seed=321)
    ctx.upload_geometry(verts, idx, ranges)
    ctx.set_instances(inst)
    orc = hits_scene(verts, idx, ranges, inst)
    rays = pool_rays(inst, verts, idx, ranges, 4000, seed=322)
    words = random_words(len(rays), seed=323)
    assert ((words & TERMINATE) != 0).sum() > 1000
    for flags, cull in ((0, 0xFF), (CULL_BACK, 0xFF), (NO_OPAQUE, 0x5A), (OPAQUE | SKIP_AABBS, 0xA5), (CULL_FRONT | CULL_NO_OPAQUE, 0x7F)):
        ref16 = oracle_lists(orc, rays, words, flags, cull, 16)
        assert (ref16[2] >= 2).sum() > 80, (flags, (ref16[2] >= 2).sum())
        for K in KS:
            for counts in (True, False):
                got = gpu_hits(ctx, rays, words, flags, cull, K, attributes=True, counts=counts)
                check_lists(orc, got, truncate(ref16, K), "words, flags %#x cull %#x K %d counts %d" % (flags, cull, K, counts))


@pytest.mark.gpu
def test_equal_t_follows_instance_and_prim_order(ctx):
    """coincident and edge-sharing triangles (edge_geometry): equal-t entries in (inst, prim) order, none lost, none twice"""
    verts, idx, ranges = edge_geometry()
    inst = edge_instances()
    ctx.upload_geometry(verts, idx, ranges)
    ctx.set_instances(inst)
    orc = hits_scene(verts, idx, ranges, inst)
    rays = edge_geometry_rays(331)
    words = random_words(len(rays), seed=332)
    ties = 0
    for flags, cull, w in ((0, 0xFF, None), (CULL_BACK, 0xFF, None), (CULL_FRONT, 0x3F, None), (0, 0xFF, words), (CULL_BACK, 0x3F, words)):
        ref16 = oracle_lists(orc, rays, w, flags, cull, 16)
        h = ref16[0]
        valid = h["inst"] >= 0
        ties += (valid[:, 1:] & (h["t"][:, 1:] == h["t"][:, :-1])).sum()
        pairs = h["inst"].astype(np.int64) * 4096 + h["prim"]
        for r in range(len(rays)):
            p = pairs[r][valid[r]]
            assert len(np.unique(p)) == len(p)
        for K in (1, 3, 8, 16):
            for counts in (True, False):
                got = gpu_hits(ctx, rays, w, flags, cull, K, attributes=K == 8, counts=counts)
                check_lists(orc, got, truncate(ref16, K), "edge flags %#x cull %#x K %d counts %d" % (flags, cull, K, counts))
    assert ties > 1000, ties


@pytest.mark.gpu
def test_count_only(ctx):
    """max_hits = 0: the counts of a listing call, without a list"""
    import torch
    verts, idx, ranges, inst = small_scene(seed=341)
    ctx.upload_geometry(verts, idx, ranges)
    ctx.set_instances(inst)
    orc = hits_scene(verts, idx, ranges, inst)
    rays = pool_rays(inst, verts, idx, ranges, 4000, seed=342)
    words = random_words(len(rays), seed=343)
    for flags, cull, w in ((0, 0xFF, None), (CULL_FRONT, 0x5A, None), (0, 0xFF, words)):
        ref = oracle_lists(orc, rays, w, flags, cull, 4)
        _, _, c4 = gpu_hits(ctx, rays, w, flags, cull, 4)
        h, a, c0 = gpu_hits(ctx, rays, w, flags, cull, 0)
        assert h is None and a is None
        assert np.array_equal(c0, c4) and np.array_equal(c0, ref[2]), (flags, cull)
        assert (c0 >= 2).sum() > 150
    res = ctx.intersect_device_hits(dev(rays), 0)
    torch.cuda.synchronize()
    assert res.t is None and res.count.shape == (len(rays),) and res.count.dtype == torch.int32


def cfg3_rays(wl, n, seed):
    """half camera rays of the cfg3 camera over a 16:9 grid, half incoherent rays from a shell about the scene"""
    rng = np.random.default_rng(seed)
    m = n // 2
    u = wl.uniforms[0]
    h = int(np.sqrt(m * 9 / 16)); w = (m + h - 1) // h
    k = np.arange(m)
    ux = (((k % w) + 0.5) / w * 2.0 - 1.0) * (w / h)
    uy = 1.0 - ((k // w) + 0.5) / h * 2.0
    R, U, F = (np.asarray(u[f][:3], np.float64) for f in ("right", "up", "forward"))
    d = ux[:, None] * R + uy[:, None] * U + 2.5 * F
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    cam = np.zeros((m, 8), np.float32)
    cam[:, 0:3] = np.asarray(u["position"][:3], np.float32); cam[:, 3] = 0.001; cam[:, 4:7] = d; cam[:, 7] = 1e4
    return np.concatenate([cam, scenes.random_rays(n - m, seed=seed + 1, target_radius=3.0)])[rng.permutation(n)]


@pytest.fixture(scope="module")
def cfg3():
    wl = workloads.make("cfg3", os.path.join(ROOT, "resources"), mesh="standin")
    g = wl.geometry
    return wl, hits_scene(g.verts, g.idx, g.ranges, wl.instances)


@pytest.mark.gpu
def test_entry0_is_the_closest_hit_1m_rays(ctx, cfg3):
    """1 M rays on the cfg3 scene (teapot and the stand-in mesh): entry 0 equals rt_intersect_device_flags' closest hit byte for byte,
    with and without counts, and with per-ray words that carry TERMINATE"""
    import torch
    wl, _ = cfg3
    wl.apply(ctx)
    n = 1 << 20
    rays = cfg3_rays(wl, n, seed=351)
    t = dev(rays)
    for words in (None, random_words(n, seed=352, flags=np.where(np.arange(n) % 3 == 0, TERMINATE, 0) | np.where(np.arange(n) % 5 == 0, CULL_BACK, 0))):
        w = None if words is None else torch.from_numpy(words.view(np.int32).copy()).to("cuda:0")
        closest = ctx.intersect_device_flags(t, words=None if w is None else (w & ~TERMINATE))
        ref = closest.hits.clone()
        for K, counts in ((1, False), (4, False), (4, True), (16, True)):
            res = ctx.intersect_device_hits(t, K, words=w, counts=counts)
            assert torch.equal(res.hits[:, 0, :], ref), (K, counts)
        torch.cuda.synchronize()
        assert (ref[:, 4] >= 0).float().mean().item() > 0.3


@pytest.mark.gpu
def test_large_scene_lists_are_candidates_in_order(ctx, cfg3):
    """on the same scene: every reported entry is one query_candidate accepts, with its t, u, v; lists strictly ordered; a 512-ray sample
    brute-forced over all triangles"""
    wl, orc = cfg3
    wl.apply(ctx)
    n = 1 << 20
    rays = cfg3_rays(wl, n, seed=361)
    K = 4
    h, a, c = gpu_hits(ctx, rays, None, 0, 0xFF, K, counts=True)
    valid = h["inst"] >= 0
    assert np.array_equal(valid.sum(axis=1), np.minimum(c, K))
    assert (c >= 2).sum() > 100_000
    ri, ji = np.nonzero(valid)
    ok, cand, _ = orc.query_candidate(rays[ri], h["inst"][ri, ji], h["prim"][ri, ji])
    assert ok.all() and cand.tobytes() == h[ri, ji].tobytes()
    a_, b_ = h[:, :-1], h[:, 1:]
    both = valid[:, 1:]
    before = (a_["t"] < b_["t"]) | ((a_["t"] == b_["t"]) & ((a_["inst"] < b_["inst"]) | ((a_["inst"] == b_["inst"]) & (a_["prim"] < b_["prim"]))))
    assert before[both].all()
    sample = np.random.default_rng(362).choice(n, 512, replace=False)
    sample = np.concatenate([sample[:256], np.nonzero(c > K)[0][:256]])
    ref = oracle_lists(orc, rays[sample], None, 0, 0xFF, K, chunk=1 << 19)
    assert h[sample].tobytes() == ref[0].tobytes() and np.array_equal(c[sample], ref[2])


@pytest.mark.gpu
def test_parity_inside_octahedra(ctx):
    """closed, convex octahedra under affine (sheared, mirrored) transforms: count % 2 == 1 exactly when the ray starts inside
    |x| + |y| + |z| < 1 in object space, on every ray the binary64 reference does not call ambiguous"""
    verts, idx, ranges = small_meshes(5)
    ranges = ranges[:1]
    inst = placed_instances(27, seed=371, spacing=5.0, n_meshes=1)
    inst["sbt_offset_and_flags"] = api.INSTANCE_FLAG_FACING_CULL_DISABLE << 24
    inst["custom_index_and_mask"] = (inst["custom_index_and_mask"] & 0xFFFFFF) | (0xFF << 24)
    ctx.upload_geometry(verts, idx, ranges)
    ctx.set_instances(inst)
    rng = np.random.default_rng(372)
    n = 20_000
    which = rng.integers(0, len(inst), n)
    p = rng.uniform(-1.4, 1.4, (n, 3))
    l1 = np.abs(p).sum(axis=1)
    keep = np.abs(l1 - 1.0) > 1e-3
    which, p, l1 = which[keep], p[keep], l1[keep]
    M = np.stack([np.asarray(inst[i]["transform"], np.float64).reshape(3, 4) for i in which])
    o = np.einsum("nij,nj->ni", M[:, :, :3], p) + M[:, :, 3]
    d = rng.normal(size=(len(o), 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((len(o), 8), np.float32)
    rays[:, 0:3] = o; rays[:, 3] = 0.0; rays[:, 4:7] = d; rays[:, 7] = 1e4
    r = ref64.query(ref64.Scene(verts, idx, ranges, inst), rays)
    sure = ~r["ambiguous"]
    assert sure.mean() > 0.95
    inside = l1 < 1.0
    assert inside[sure].sum() > 1000 and (~inside[sure]).sum() > 1000
    for K in (0, 2):
        _, _, c = gpu_hits(ctx, rays, None, 0, 0xFF, K)
        assert np.array_equal((c[sure] % 2) == 1, inside[sure]), K
        assert (c[sure] > 2).sum() > 100   # rays that pass through other octahedra too


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "1"])
def test_scene_sources_and_builders(builder, monkeypatch):
    """host and device instance records, a BLAS refit with device instances after it, under the host and the device BLAS builder"""
    import torch
    from tests.test_blas_refit import deform, with_mesh
    verts, idx, ranges, inst = small_scene(seed=381)
    geom = types.SimpleNamespace(verts=verts, idx=idx, ranges=ranges)
    rng = np.random.default_rng(382)
    moved = inst.copy()
    moved["transform"][:, [3, 7, 11]] += rng.uniform(-0.3, 0.3, (len(inst), 3)).astype(np.float32)
    rays = pool_rays(inst, verts, idx, ranges, 2400, seed=383)
    words = random_words(len(rays), seed=384)
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
                orc = hits_scene(verts, idx, ranges, records)
                for flags, cull, K in ((0, 0xFF, 8), (CULL_BACK, 0x5A, 3)):
                    ref = oracle_lists(orc, rays, words, flags, cull, K)
                    for counts in (True, False):
                        check_lists(orc, gpu_hits(c, rays, words, flags, cull, K, attributes=True, counts=counts), ref,
                                    "%s records, update %d, builder %s" % (source, update, builder))
        t = deform(geom, 0, amp=0.2)
        torch.cuda.synchronize()
        c.refit_blas_device(0, t)
        torch.cuda.synchronize()
        c.set_instances_device(dev_inst(inst))
        orc = hits_scene(with_mesh(geom, verts, 0, t), idx, ranges, inst)
        ref = oracle_lists(orc, rays, words, 0, 0xFF, 8)
        for counts in (True, False):
            check_lists(orc, gpu_hits(c, rays, words, 0, 0xFF, 8, attributes=True, counts=counts), ref, "refit, builder %s" % builder)
    finally:
        c.close()


@pytest.mark.gpu
def test_stream_order_and_later_instances(ctx):
    """rays written by a slow queue on a side stream are read in order; an rt_set_instances after the call does not change its result"""
    import torch
    verts, idx, ranges, inst = small_scene(seed=391)
    other = placed_instances(32, seed=392, spacing=3.0)
    ctx.upload_geometry(verts, idx, ranges)
    ctx.set_instances(inst)
    orc = hits_scene(verts, idx, ranges, inst)
    rays_np = pool_rays(inst, verts, idx, ranges, 4000, seed=393)
    ref = oracle_lists(orc, rays_np, None, 0, 0xFF, 4)
    src = dev(rays_np)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = slow_queue(torch, 12)
        rays = (src + (a[0, 0] != a[0, 0]).to(torch.float32) * 0).contiguous()   # made behind the queue, on s
        res = ctx.intersect_device_hits(rays, 4, attributes=True, stream=s)
        rays.zero_()                                                             # overwritten right after the call
        hits, attr, count = res.hits.clone(), res.attr.clone(), res.count.clone()
    ctx.set_instances(other)   # the other TLAS parity, then the query's own: waits for the query
    ctx.set_instances(other)
    s.synchronize()
    got = (hits.cpu().numpy().view(HIT_DTYPE).reshape(len(rays_np), 4), attr.cpu().numpy(), count.cpu().numpy().view(np.uint32))
    check_lists(orc, got, ref, "side stream")
    # the null-stream path of the wrapper
    ctx.set_instances(inst)
    torch.cuda.synchronize()
    a = slow_queue(torch)
    rays = (src + (a[0, 0] != a[0, 0]).to(torch.float32) * 0).contiguous()
    res = ctx.intersect_device_hits(rays, 4)
    rays.zero_()
    check_lists(orc, res.numpy(), ref, "null stream")


@pytest.mark.gpu
def test_frames_beside_a_hits_query():
    """a frame rendered before, during (on another slot) and after a hits query is the same frame: the query shares no workspace with frames"""
    import torch
    from tests.test_ray_query import W, H, two_objects
    base = RtContext(0)
    slot = base.frame_slot()
    try:
        sp = two_objects(base)
        slot.set_instances(sp.instances)
        slot.set_uniforms(sp.uniforms)
        before = base.trace(W, H)[0]
        orc = hits_scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances)
        rays_np = mixed_rays(2000, seed=401)
        ref = oracle_lists(orc, rays_np, None, 0, 0xFF, 4)
        rays = dev(rays_np)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        slot.trace_async(W, H)
        with torch.cuda.stream(s):
            slow_queue(torch, 4)
            res = base.intersect_device_hits(rays, 4, stream=s)
        during, _ = slot.trace_wait()
        after = base.trace(W, H)[0]
        s.synchronize()
        assert np.array_equal(during.view(np.uint32), before.view(np.uint32))
        assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
        check_lists(orc, res.numpy(), ref, "beside frames")
    finally:
        slot.close()
        base.close()


def _raw(c, n, rays, words, flags, cull, k, hits, attr, counts):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_intersect_device_hits(c.h, n, p(rays), p(words), flags, cull, k, p(hits), p(attr), p(counts), None)


@pytest.mark.gpu
def test_error_statuses():
    import torch
    from tests.test_blas_refit import span
    rays_np = mixed_rays(1000, seed=411)
    rays = dev(rays_np)
    n = rays.shape[0]
    hits = torch.empty((n * 16 + 1, 5), dtype=torch.int32, device="cuda:0")
    attr = torch.empty((n * 16 + 1, 8), dtype=torch.int32, device="cuda:0")
    cnt = torch.empty((n + 1,), dtype=torch.int32, device="cuda:0")
    words = torch.full((n + 1,), -16777216, dtype=torch.int32, device="cuda:0")
    R_, H_, A_, C_, W_ = rays.data_ptr(), hits.data_ptr(), attr.data_ptr(), cnt.data_ptr(), words.data_ptr()
    c = RtContext(0)

    def err(args, code, text):
        assert _raw(c, *args) == code, args
        msg = c.L.rt_last_error(c.h).decode()
        assert text in msg, (args, msg)

    try:
        err((n, R_, 0, 0, 0xFF, 4, H_, 0, 0), RT_ERR_NOT_READY, "")   # no geometry
        sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
        c.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        err((n, R_, 0, 0, 0xFF, 4, H_, 0, 0), RT_ERR_NOT_READY, "")   # no TLAS
        c.set_instances(sp.instances)
        c.set_uniforms(sp.uniforms)
        orc = hits_scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances)
        ref = oracle_lists(orc, rays_np, None, 0, 0xFF, 4)

        def ok():
            check_lists(orc, c.intersect_device_hits(rays, 4).numpy(), ref, "after an error")

        ok()
        bad = [
            ((n, R_, 0, 0, 0xFF, 17, H_, 0, 0), "max_hits must be 0..16"),
            ((n, R_, 0, 0, 0xFF, 0, 0, 0, 0), "max_hits 0 counts only"),
            ((n, R_, 0, 0, 0xFF, 0, H_, 0, C_), "max_hits 0 counts only"),
            ((n, R_, 0, 0, 0xFF, 0, 0, A_, C_), "max_hits 0 counts only"),
            ((n, R_, 0, TERMINATE, 0xFF, 4, H_, 0, 0), "TERMINATE_ON_FIRST_HIT"),
            ((n, R_, 0, TERMINATE | OPAQUE, 0xFF, 4, H_, 0, C_), "TERMINATE_ON_FIRST_HIT"),
            ((n, R_, 0, 0x400, 0xFF, 4, H_, 0, 0), "bits outside 0x3FF"),
            ((n, R_, 0, 0, 0x100, 4, H_, 0, 0), "bits outside 0x3FF"),
            ((n, R_, 0, OPAQUE | NO_OPAQUE, 0xFF, 4, H_, 0, 0), "at most one of OPAQUE"),
            ((n, R_, 0, CULL_BACK | CULL_FRONT, 0xFF, 4, H_, 0, 0), "CULL_BACK_FACING with CULL_FRONT_FACING"),
            ((n, R_, 0, api.RAY_FLAG_SKIP_TRIANGLES | SKIP_AABBS, 0xFF, 4, H_, 0, 0), "SKIP_TRIANGLES with SKIP_AABBS"),
            ((n, R_, 0, api.RAY_FLAG_SKIP_TRIANGLES | CULL_BACK, 0xFF, 4, H_, 0, 0), "SKIP_TRIANGLES with SKIP_AABBS or a facing cull"),
            ((0xFFFFFF00, R_, 0, 0, 0xFF, 1, H_, 0, 0), "too many rays"),
            ((0x10000000, R_, 0, 0, 0xFF, 16, H_, 0, 0), "n * max_hits"),
            ((n, 0, 0, 0, 0xFF, 4, H_, 0, 0), "null ray/hit pointers"),
            ((n, R_, 0, 0, 0xFF, 4, 0, 0, C_), "null ray/hit pointers"),
            ((n, R_ + 4, 0, 0, 0xFF, 4, H_, 0, 0), "aligned"),
            ((n, R_, W_ + 2, 0, 0xFF, 4, H_, 0, 0), "aligned"),
            ((n, R_, 0, 0, 0xFF, 4, H_ + 2, 0, 0), "aligned"),
            ((n, R_, 0, 0, 0xFF, 4, H_, A_ + 4, 0), "aligned"),
            ((n, R_, 0, 0, 0xFF, 4, H_, 0, C_ + 2), "aligned"),
        ]
        host_buf = np.zeros((n * 16 + 1, 8), np.float32)
        pinned = torch.zeros((n * 16, 8), dtype=torch.float32).pin_memory()
        for ptr in ((host_buf.ctypes.data + 15) & ~15, pinned.data_ptr()):   # (16-byte aligned: only the memory kind is wrong)
            bad += [((n, ptr, 0, 0, 0xFF, 4, H_, 0, 0), "device memory of the context's GPU"),
                    ((n, R_, 0, 0, 0xFF, 4, ptr, 0, 0), "device memory of the context's GPU"),
                    ((n, R_, ptr, 0, 0xFF, 4, H_, 0, 0), "device memory of the context's GPU"),
                    ((n, R_, 0, 0, 0xFF, 4, H_, 0, ptr), "device memory of the context's GPU"),
                    ((n, R_, 0, 0, 0xFF, 4, H_, ptr, 0), "device memory of the context's GPU")]
        for args, text in bad:
            err(args, RT_ERR_INVALID_ARGUMENT, text)
            ok()
        # n == 0 enqueues nothing and needs no pointers
        assert _raw(c, 0, 0, 0, 0, 0xFF, 4, 0, 0, 0) == 0
        # the Python checks
        with pytest.raises(ValueError):
            c.intersect_device_hits(rays, 17)
        with pytest.raises(ValueError):
            c.intersect_device_hits(rays, 0, counts=False)
        with pytest.raises(RtError) as e:
            c.intersect_device_hits(rays, 4, ray_flags=TERMINATE)
        assert e.value.code == RT_ERR_INVALID_ARGUMENT and "TERMINATE_ON_FIRST_HIT" in str(e.value)
        with pytest.raises(ValueError):
            c.intersect_device_hits(rays.cpu(), 4)
        ok()
        # not ready: a stale TLAS after a BLAS refit, then a frame batch
        ff, nf = span(sp.geom, 1)
        v = torch.from_numpy(sp.geom.verts[ff:ff + nf].copy()).to("cuda:0")
        torch.cuda.synchronize()
        c.refit_blas_device(1, v)
        err((n, R_, 0, 0, 0xFF, 4, H_, 0, 0), RT_ERR_NOT_READY, "")
        c.set_instances(sp.instances)
        ok()
        c.set_batch(np.stack([sp.instances, sp.instances]), np.stack([sp.uniforms, sp.uniforms]).reshape(-1))
        err((n, R_, 0, 0, 0xFF, 4, H_, 0, 0), RT_ERR_NOT_READY, "")
        c.set_instances(sp.instances)
        ok()
    finally:
        c.close()
    # trace_variant != 0 (alt library only: the product refuses the parameter itself)
    a = RtContext(0, variant="alt")
    try:
        sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
        a.set_param("blas_builder", 0)
        a.set_param("trace_variant", 1)
        a.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        a.set_instances(sp.instances)
        c = a
        err((n, R_, 0, 0, 0xFF, 4, H_, 0, 0), RT_ERR_INVALID_ARGUMENT, "trace_variant 0")
        a.set_param("trace_variant", 0)
        a.set_instances(sp.instances)
        check_lists(orc, a.intersect_device_hits(rays, 4).numpy(), ref, "alt library")
    finally:
        a.close()
