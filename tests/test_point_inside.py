"""rt_point_inside_device, rt_point_inside and rt_signed_distance_device (include/rt_api.h; DESIGN.md §5 "Inside / outside").

CPU: the exports, the direction table, the vote restated (tests/inside_reference.py) and checked by hand, and the experiment that chose
the vote: on closed meshes under rotated, sheared and mirrored instances, with points from which a table direction runs through a vertex
or an edge, every single direction gives wrong parities, the vote over three equals the binary64 winding number's parity everywhere, and
the vote over five equals the vote over three.

GPU: the crossing counts equal rt_intersect_device_hits' counts of the composed rays byte for byte and the oracle's brute-force counts;
the words equal the restated vote with and without counts; across builders, record sources, refits, cull masks, deep trees, far offsets
and invalid points; the signed distance equals rt_closest_point_device apart from the sign bit, which is bit 0 of the word."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import closest_reference as cr
from tests import inside_reference as ir
from tests import scenes
from tests.test_closest_point import scene_box, small_scene, surface_points, teapot_scene
from tests.test_ray_query import PATHS, dev_inst, slow_queue
from tests.test_ray_query_oracle import oracle_scene, use_builder
from vulkan_raytracing_amd import RtContext, api, workloads
from vulkan_raytracing_amd.api import RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
N_DIRS = (1, 3, 5)


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_exports_abi_and_null_context():
    for name in ("rt_point_inside_device", "rt_point_inside", "rt_signed_distance_device"):
        assert name in api.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^#define RT_INSIDE_MAX_DIRS 5$", hdr, re.M)
    assert re.search(r"^int rt_point_inside_device\(rt_ctx\* ctx, size_t n, const void\* d_points4, uint32_t cull_mask, uint32_t n_dirs,\s+"
                     r"void\* d_inside, void\* d_counts, void\* hip_stream\);", hdr, re.M)
    assert re.search(r"^int rt_point_inside\(rt_ctx\* ctx, size_t n, const float\* points4_host, uint32_t cull_mask, uint32_t n_dirs,\s+"
                     r"uint32_t\* inside_host, uint32_t\* counts_host, int counting, rt_stats\* stats\);", hdr, re.M)
    assert re.search(r"^int rt_signed_distance_device\(rt_ctx\* ctx, size_t n, const void\* d_points4, uint32_t cull_mask, uint32_t n_dirs,\s+"
                     r"void\* d_hits, void\* d_attr, void\* d_inside, void\* hip_stream\);", hdr, re.M)
    L = api.lib()
    assert L.rt_abi_version() == 7
    assert L.rt_point_inside_device(None, 0, None, 0xFF, 3, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_point_inside_device(None, 64, None, 0xFF, 3, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_point_inside(None, 0, None, 0xFF, 3, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_signed_distance_device(None, 0, None, 0xFF, 3, None, None, None, None) == RT_ERR_INVALID_ARGUMENT
    for name in ("point_inside_device", "point_inside", "signed_distance_device"):
        assert hasattr(RtContext, name)


def test_direction_table_equals_the_header():
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    m = re.search(r"^#define RT_INSIDE_DIRS (.*)$", hdr, re.M)
    lit = re.findall(r"-?\d+\.\d+(?=f)", m.group(1))
    assert len(lit) == 15
    table = np.array([float(x) for x in lit]).reshape(5, 3)
    assert np.array_equal(table, np.array(api.INSIDE_DIRS)) and len(api.INSIDE_DIRS) == 5
    want = [(0.36, 0.48, 0.8), (-0.8, 0.36, -0.48), (0.48, -0.8, -0.36), (-0.6, -0.64, 0.48), (0.64, -0.48, 0.6)]
    assert [tuple(r) for r in api.INSIDE_DIRS] == want
    assert np.array_equal(ir.DIRS, np.array(want, np.float32))
    # generic: no zero component, no two components of equal magnitude within a direction, no two directions parallel or opposite
    a = np.abs(table)
    assert (a > 0).all() and all(len(set(r)) == 3 for r in a.tolist())
    u = table / np.linalg.norm(table, axis=1, keepdims=True)
    assert (np.abs(u @ u.T)[~np.eye(5, dtype=bool)] < 0.99).all()


def test_vote_restatement_by_hand():
    """every parity pattern of 3 and 5 directions, written out: (odd votes, directions taken) under the early stop"""
    w = lambda bit, odd, taken: bit | (odd << 8) | (taken << 16)   # noqa: E731
    # n_dirs 1
    assert ir.words([[4], [7]], 1, False).tolist() == [w(0, 0, 1), w(1, 1, 1)] == ir.words([[4], [7]], 1, True).tolist()
    # n_dirs 3, early stop: two equal votes decide
    by_hand3 = {(0, 0, 0): w(0, 0, 2), (0, 0, 1): w(0, 0, 2), (0, 1, 0): w(0, 1, 3), (0, 1, 1): w(1, 2, 3),
                (1, 0, 0): w(0, 1, 3), (1, 0, 1): w(1, 2, 3), (1, 1, 0): w(1, 2, 2), (1, 1, 1): w(1, 2, 2)}
    pats = sorted(by_hand3)
    assert len(pats) == 8
    assert ir.words(pats, 3, False).tolist() == [by_hand3[p] for p in pats]
    assert ir.words(pats, 3, True).tolist() == [w(int(sum(p) >= 2), sum(p), 3) for p in pats]
    # counts, not parities, come in: 2 and 4 are even, 3 and 5 odd
    assert ir.words([[2, 5, 3], [4, 4, 9]], 3, False).tolist() == [w(1, 2, 3), w(0, 0, 2)]
    # n_dirs 5: the walk stops at the first direction t after which odd or even holds 3 votes
    pats = [tuple((i >> (4 - k)) & 1 for k in range(5)) for i in range(32)]
    early = ir.words(pats, 5, False)
    full = ir.words(pats, 5, True)
    for p, e, f in zip(pats, early.tolist(), full.tolist()):
        t = next(t for t in range(3, 6) if sum(p[:t]) >= 3 or t - sum(p[:t]) >= 3)
        assert e == w(int(sum(p[:t]) >= 3), sum(p[:t]), t), p
        assert f == w(int(sum(p) >= 3), sum(p), 5), p
        assert (e & 1) == (f & 1)
    by_hand5 = {(0, 0, 0, 1, 1): w(0, 0, 3), (1, 1, 1, 0, 0): w(1, 3, 3), (1, 0, 1, 0, 1): w(1, 3, 5), (0, 1, 0, 1, 0): w(0, 2, 5),
                (1, 1, 0, 1, 0): w(1, 3, 4), (0, 1, 0, 0, 1): w(0, 1, 4)}
    assert ir.words(list(by_hand5), 5, False).tolist() == list(by_hand5.values())


def test_one_direction_is_not_enough_and_three_are():
    """the oracle's crossing counts (query_candidate over all 848 triangles, tmax = +inf) on 38 088 points, 34 488 of them adversarial:
    each of D0..D2 alone is wrong on at least 100 points, the 3-vote equals the binary64 winding parity on every point, the 5-vote
    equals the 3-vote, and no point is ambiguous (none lies on a surface)"""
    e = ir.experiment()
    c, kept, truth = e["counts"], e["kept"], e["truth"]
    assert e["tc"].sum() == 848 and len(e["points"]) == 38088 and e["adv"].sum() == 34488
    assert (~kept).mean() <= 0.02
    assert 0.1 < truth[kept].mean() < 0.5   # (both answers occur)
    wrong = [int((((c[:, k] & 1) != truth) & kept).sum()) for k in range(5)]
    print("wrong parities per direction:", wrong, "dropped:", int((~kept).sum()))
    assert min(wrong[:3]) >= 100
    w1, w3, w5 = (ir.words(c, k, False) for k in N_DIRS)
    assert np.array_equal((w1 & 1), c[:, 0] & 1)
    assert np.array_equal((w3 & 1)[kept], truth[kept])
    assert np.array_equal(w5 & 1, w3 & 1)
    assert np.array_equal(ir.words(c, 3, True) & 1, w3 & 1) and np.array_equal(ir.words(c, 5, True) & 1, w5 & 1)


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_inside_kernels_use_no_scratch(target):
    """exactly two new walk kernels, k_point_inside and its counting form, and k_sign_distance, in both libraries: no scratch, no spills,
    and the walks within the record-level budget (>= 4 waves per SIMD)"""
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    walk = [(n, r) for n, r in kernels.items() if "k_point_inside" in n]
    sign = [(n, r) for n, r in kernels.items() if "k_sign_distance" in n]
    assert len(walk) == 2 and len(sign) == 1 and sum("k_point_inside_count" in n for n, _ in walk) == 1, "\n".join(kernels)
    for name, r in walk + sign:
        assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
    for name, r in walk:
        assert int(r["Occupancy"]) >= 4, (name, r)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


def dev(p):
    import torch
    return torch.from_numpy(np.ascontiguousarray(p, np.float32).reshape(-1, 4)).to("cuda:0")


def load(c, parts):
    verts, idx, ranges, inst = parts
    c.upload_geometry(verts, idx, ranges)
    c.set_instances(inst)


def gpu_inside(c, pts, n_dirs=3, cull=0xFF, counts=False):
    """(words uint32 (n,), counts uint32 (n, n_dirs) or None)"""
    import torch
    res = c.point_inside_device(dev(pts), n_dirs=n_dirs, cull_mask=cull, counts=counts)
    torch.cuda.synchronize()
    return res.numpy()


def gpu_composed(c, pts, n_dirs, cull=0xFF):
    """what a torch user does today: the count-only all-hits query over the n * n_dirs composed rays -> uint32 (n, n_dirs)"""
    import torch
    rays = torch.from_numpy(ir.compose_rays(pts, n_dirs)).to("cuda:0")
    res = c.intersect_device_hits(rays, 0, ray_flags=0, cull_mask=cull)
    torch.cuda.synchronize()
    return res.numpy()[2].reshape(-1, n_dirs)


def check(c, pts, n_dirs, ref, what, cull=0xFF, composed=True):
    """counts against the composed query byte for byte and against `ref` (n, >= n_dirs; or None); the words against the restated vote
    with and without counts"""
    w_all, cnt = gpu_inside(c, pts, n_dirs, cull, counts=True)
    w_early, none = gpu_inside(c, pts, n_dirs, cull, counts=False)
    assert none is None and cnt.shape == (len(pts), n_dirs) and cnt.dtype == np.uint32
    if composed:
        comp = gpu_composed(c, pts, n_dirs, cull)
        assert cnt.tobytes() == comp.tobytes(), (what, np.nonzero((cnt != comp).any(axis=1))[0][:5])
    if ref is not None:
        r = np.ascontiguousarray(ref[:, :n_dirs])
        assert np.array_equal(cnt, r), (what, np.nonzero((cnt != r).any(axis=1))[0][:5])
    assert np.array_equal(w_all, ir.words(cnt, n_dirs, True)), what
    assert np.array_equal(w_early, ir.words(cnt, n_dirs, False)), what
    assert np.array_equal(w_all & 1, w_early & 1), what
    return w_early, cnt


@pytest.mark.gpu
@pytest.mark.parametrize("n_dirs", N_DIRS)
def test_experiment_scene(ctx, n_dirs):
    """the CPU experiment's scene and points: counts = composed query = oracle; words = restatement; bit 0 = the winding parity"""
    e = ir.experiment()
    load(ctx, e["parts"])
    w, cnt = check(ctx, e["points"], n_dirs, e["counts"], "experiment, %d directions" % n_dirs)
    if n_dirs >= 3:
        assert np.array_equal((w & 1)[e["kept"]], e["truth"][e["kept"]])
    else:
        assert ((w & 1) != e["truth"])[e["kept"]].sum() >= 100   # (one ray is not enough on the GPU either)
    taken = (w >> 16) & 0xFF
    assert set(np.unique(taken)) <= set(range(n_dirs // 2 + 1, n_dirs + 1)) and (n_dirs == 1 or (taken < n_dirs).mean() > 0.5)
    for n in (1, 63, 64, 65, 4097):   # (the chunk refill)
        sel = np.arange(n) * 9 % len(e["points"])
        check(ctx, e["points"][sel], n_dirs, e["counts"][sel], "%d points" % n, composed=False)


def small_points(sc, n, seed):
    """uniform in the scene's box, near the surface, and behind vertices along D0..D2; w = 7 (ignored)"""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(sc)
    vol = lo + rng.uniform(size=(n, 3)) * (hi - lo)
    near = surface_points(sc, n, rng, 0.3)
    k = rng.integers(0, sc.n_tris, n // 2)
    behind = sc.A[k] - rng.uniform(0.2, 2.0, (n // 2, 1)) * ir.DIRS[rng.integers(0, 3, n // 2)].astype(np.float64)
    p = np.concatenate([vol, near, behind]).astype(np.float32)
    return np.concatenate([p, np.full((len(p), 1), 7.0, np.float32)], axis=1)


_SMALL = {}


def small(offset=0.0):
    """small_scene (octahedra and triangle soups, eight masks), its points and the oracle's counts under every cull mask used, once"""
    if offset not in _SMALL:
        parts = small_scene(offset=offset)
        verts, idx, ranges, inst = parts
        sc = cr.Scene(*parts)
        orc = oracle_scene(*parts)
        pts = small_points(sc, 1200, seed=311)
        tc = ir.tri_counts(ranges, inst)
        ref = {cull: ir.oracle_counts(orc, tc, pts, 5, cull) for cull in ((0xFF, 0x01, 0x0F, 0x00) if offset == 0.0 else (0xFF,))}
        _SMALL[offset] = (parts, sc, pts, ref)
    return _SMALL[offset]


@pytest.mark.gpu
@pytest.mark.parametrize("n_dirs", N_DIRS)
def test_small_scene_and_cull_masks(ctx, n_dirs):
    """open soups and mixed instance masks: the counts are the composed query's and the oracle's under every cull mask; an instance
    left out does not count, cull mask 0 gives zeros"""
    parts, sc, pts, ref = small()
    load(ctx, parts)
    for cull in (0xFF, 0x01, 0x0F, 0x00):
        w, cnt = check(ctx, pts, n_dirs, ref[cull], "small, cull %#x" % cull, cull=cull)
        assert (cnt <= ref[0xFF][:, :n_dirs]).all()
        if cull == 0:
            assert (cnt == 0).all() and (w & 0xFFFF == 0).all() and ((w >> 16) == n_dirs // 2 + 1).all()
    assert (ref[0xFF] > 0).mean() > 0.2 and (ref[0x01] != ref[0xFF]).any() and (ref[0x0F] != ref[0x01]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "unset", "1", "2"])
def test_tree_independence(builder, monkeypatch):
    """the same points over blas_builder 0 and RT_GPU_BVH_ALGO unset / 1 / 2, host and device instance records with their updates: every
    output equals the oracle's brute force, so they are byte-identical to each other"""
    import torch
    parts, sc, pts, ref = small()
    verts, idx, ranges, inst = parts
    rng = np.random.default_rng(72)
    moved = inst.copy()
    moved["transform"][:, [3, 7, 11]] += rng.uniform(-0.3, 0.3, (len(inst), 3)).astype(np.float32)
    if "moved" not in _SMALL:
        _SMALL["moved"] = ir.oracle_counts(oracle_scene(verts, idx, ranges, moved), ir.tri_counts(ranges, inst), pts, 5)
    r0, r1 = ref[0xFF], _SMALL["moved"]
    assert (r0 != r1).any()
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
                check(c, pts, 5, r, "%s records, update %d, builder %s" % (source, update, builder), composed=False)
    finally:
        c.close()


@pytest.mark.gpu
def test_refit_then_tlas_update_equals_a_fresh_build():
    import torch
    from tests.test_blas_refit import deform, with_mesh
    parts, sc, pts, ref = small()
    verts, idx, ranges, inst = parts
    geom = types.SimpleNamespace(verts=verts, idx=idx, ranges=ranges)
    src = dev(pts)
    c, fresh = RtContext(0), RtContext(0)
    try:
        load(c, parts)
        t = deform(geom, 0, amp=0.2)
        torch.cuda.synchronize()
        c.refit_blas_device(0, t)
        torch.cuda.synchronize()
        word = torch.empty((len(pts),), dtype=torch.int32, device="cuda:0")
        rc = c.L.rt_point_inside_device(c.h, len(pts), ctypes.c_void_p(src.data_ptr()), 0xFF, 3, ctypes.c_void_p(word.data_ptr()), None, None)
        assert rc == RT_ERR_NOT_READY
        c.set_instances_device(dev_inst(inst))
        v2 = with_mesh(geom, verts, 0, t)
        load(fresh, (v2, idx, ranges, inst))
        want = ir.oracle_counts(oracle_scene(v2, idx, ranges, inst), ir.tri_counts(ranges, inst), pts, 3)
        assert (want != ref[0xFF][:, :3]).any()
        got = check(c, pts, 3, want, "after the refit")
        new = check(fresh, pts, 3, want, "fresh build")
        assert got[0].tobytes() == new[0].tobytes() and got[1].tobytes() == new[1].tobytes()
    finally:
        c.close()
        fresh.close()


@pytest.mark.gpu
def test_deep_tree(ctx):
    """six teapots (13 536 triangles each, the deepest BLAS of the test scenes): 4 097 points against the composed query, the first 96
    against the oracle"""
    parts = teapot_scene()
    verts, idx, ranges, inst = parts
    load(ctx, parts)
    sc = cr.Scene(*parts)
    pts = small_points(sc, 1639, seed=321)[:4097]
    assert len(pts) == 4097
    w, cnt = check(ctx, pts, 3, None, "teapots")
    sel = np.arange(96) * 41
    cull = 0xFF
    want = ir.oracle_counts(oracle_scene(*parts), ir.tri_counts(ranges, inst), pts[sel], 3, cull)
    assert np.array_equal(cnt[sel], want) and (want > 0).any()


@pytest.mark.gpu
def test_invalid_points_and_far_offsets(ctx):
    """NaN and +-inf in each coordinate: word 0 and counts 0, whatever their neighbours do; w is ignored (NaN, inf, negative); the
    scene 10 000 units from the origin (the far-ray path of the walk) against the oracle and the composed query"""
    parts, sc, pts, ref = small()
    load(ctx, parts)
    q = pts[:200].copy()
    bad = []
    for i, (col, val) in enumerate((c, v) for c in range(3) for v in (np.nan, np.inf, -np.inf)):
        q[7 * i + 3, col] = val
        bad.append(7 * i + 3)
    q[100, 3] = np.nan; q[101, 3] = np.inf; q[102, 3] = -1.0
    for n_dirs in N_DIRS:
        for counts in (True, False):
            w, cnt = gpu_inside(ctx, q, n_dirs, counts=counts)
            assert (w[bad] == 0).all()
            ok = np.setdiff1d(np.arange(len(q)), bad)
            r = ref[0xFF][:200][:, :n_dirs]
            assert np.array_equal(w[ok], ir.words(r[ok], n_dirs, counts))
            if counts:
                assert (cnt[bad] == 0).all() and np.array_equal(cnt[ok], r[ok])
    allbad = np.full((130, 4), np.nan, np.float32)   # (whole chunks of invalid points)
    w, cnt = gpu_inside(ctx, allbad, 3, counts=True)
    assert (w == 0).all() and (cnt == 0).all()
    parts, sc, pts, ref = small(offset=10000.0)
    load(ctx, parts)
    assert np.abs(pts[:, :3]).min(axis=0).max() > 5e3
    for n_dirs in N_DIRS:
        check(ctx, pts, n_dirs, ref[0xFF], "small+10000, %d directions" % n_dirs)
    assert (ref[0xFF] > 0).mean() > 0.1


def sign_split(h):
    """(the records with the sign bit of t cleared, the sign bits)"""
    raw = np.ascontiguousarray(h).view(np.uint32).reshape(len(h), 5).copy()
    sign = raw[:, 0] >> 31
    raw[:, 0] &= 0x7FFFFFFF
    return raw, sign


@pytest.mark.gpu
@pytest.mark.parametrize("n_dirs", N_DIRS)
def test_signed_distance(ctx, n_dirs):
    """rt_closest_point_device's records and attributes byte for byte apart from the sign bit of t, which is bit 0 of
    rt_point_inside_device's word: with r_max = inf, with an r_max below the distance (the miss record becomes -r_max), and unchanged
    for records that are not valid closest-point queries; the words with and without d_inside"""
    import torch
    e = ir.experiment()
    load(ctx, e["parts"])
    sel = np.arange(6000) * 6 % len(e["points"])
    pts = e["points"][sel].copy()
    src = dev(pts)
    cp = ctx.closest_point_device(src, attributes=True)
    torch.cuda.synchronize()
    ch, ca = cp.numpy()
    tight = pts.copy()
    tight[:, 3] = np.where(np.arange(len(pts)) % 2 == 0, ch["t"] * np.float32(0.5), ch["t"] * np.float32(1.5))
    tight[5, 3] = -1.0; tight[6, 3] = np.nan; tight[7, 0] = np.nan; tight[8, 3] = np.float32(-0.0); tight[9, 3] = 0.0
    for name, p in (("inf", pts), ("tight", tight)):
        t = dev(p)
        cp = ctx.closest_point_device(t, attributes=True)
        plain = ctx.signed_distance_device(t, n_dirs=n_dirs, attributes=True)
        with_words = ctx.signed_distance_device(t, n_dirs=n_dirs, words=True)
        ins = ctx.point_inside_device(t, n_dirs=n_dirs)
        torch.cuda.synchronize()
        (ch, ca), (sh, sa), (wh, _), (w, _) = cp.numpy(), plain.numpy(), with_words.numpy(), ins.numpy()
        assert plain.word is None and np.array_equal(with_words.word.cpu().numpy().view(np.uint32), w), name
        assert sh.tobytes() == wh.tobytes() and sa.tobytes() == ca.tobytes(), name
        raw, sign = sign_split(sh)
        craw, csign = sign_split(ch)
        valid = np.isfinite(p[:, :3]).all(axis=1) & (p[:, 3] >= 0)
        assert np.array_equal(raw[valid], craw[valid]) and np.array_equal(sign[valid], csign[valid] | (w[valid] & 1)), name
        assert sh[~valid].tobytes() == ch[~valid].tobytes(), name
        assert np.array_equal(ins.inside.cpu().numpy(), (w & 1).astype(bool))
        miss = sh["inst"] < 0
        inside = (w & 1) == 1
        if name == "tight":
            assert (~valid).sum() == 3 and (w[7] == 0) and (miss & inside & valid).sum() > 100 and (~miss & inside).sum() > 100
            m = miss & inside & valid
            assert np.array_equal(sh["t"][m], -p[m, 3]) and (sh["t"][miss & ~inside & valid] == p[miss & ~inside & valid, 3]).all()
            assert valid[8] and valid[9] and csign[8] == 1 and sign[8] == 1 and sign[9] == (w[9] & 1)   # (r_max = -0.0 and 0 are valid radii)
        else:
            assert valid.all() and not miss.any() and 0.1 < inside.mean() < 0.6
            assert (sh["t"][inside] <= 0).all() and (np.signbit(sh["t"]) == inside).all()
            if n_dirs >= 3:
                kept = e["kept"][sel]
                assert np.array_equal(np.signbit(sh["t"])[kept], e["truth"][sel][kept] == 1)


@pytest.mark.gpu
def test_plumbing(ctx):
    """host form = device form; the counting form returns counters and the same words; out= reuse; a caller's stream with the points
    written behind a slow queue and overwritten right after the call; n == 0"""
    import torch
    e = ir.experiment()
    load(ctx, e["parts"])
    sel = np.arange(3000) * 11 % len(e["points"])
    pts, ref = e["points"][sel], e["counts"][sel]
    w3, wall = ir.words(ref, 3, False), ir.words(ref, 3, True)
    hw, hc, st = ctx.point_inside(pts)
    assert np.array_equal(hw, w3) and hc is None
    assert st.node_visits == 0 and st.tri_tests == 0 and st.bvh_node_bytes > 0 and st.bvh_tri_bytes > 0 and st.ms_trace_closest > 0
    hw, hc, st = ctx.point_inside(pts, counts=True, counting=True)
    assert np.array_equal(hw, wall) and np.array_equal(hc, ref[:, :3])
    assert st.node_visits > 0 and st.tri_tests >= int(ref[:, :3].sum())
    hw, hc, st5 = ctx.point_inside(pts, n_dirs=5, counting=True)
    assert np.array_equal(hw, ir.words(ref, 5, False)) and hc is None
    hw1, _, st1 = ctx.point_inside(pts, n_dirs=1, counting=True)
    assert np.array_equal(hw1, ir.words(ref, 1, False)) and 0 < st1.tri_tests < st.tri_tests   # (the early stop walks less)
    assert (ctx.point_inside(pts, cull_mask=0)[0] & 0xFFFF == 0).all()
    for n in (1, 63, 64, 65):
        assert np.array_equal(ctx.point_inside(pts[:n], counts=True)[1], ref[:n, :3])
    # out= reuse
    src = dev(pts)
    word = torch.empty((len(pts),), dtype=torch.int32, device="cuda:0"); count = torch.empty((len(pts), 3), dtype=torch.int32, device="cuda:0")
    res = ctx.point_inside_device(src, counts=True, out=(word, count))
    assert res.word.data_ptr() == word.data_ptr() and res.count.data_ptr() == count.data_ptr()
    torch.cuda.synchronize()
    assert np.array_equal(res.numpy()[0], wall) and np.array_equal(res.numpy()[1], ref[:, :3])
    res = ctx.point_inside_device(src, out=(word, None))
    torch.cuda.synchronize()
    assert res.count is None and np.array_equal(res.numpy()[0], w3)
    with pytest.raises(ValueError):
        ctx.point_inside_device(src, out=(word[:-1], None))
    with pytest.raises(ValueError):
        ctx.point_inside_device(src, counts=True, out=(word, torch.empty((len(pts), 5), dtype=torch.int32, device="cuda:0")))
    hits = torch.empty((len(pts), 5), dtype=torch.int32, device="cuda:0"); attr = torch.empty((len(pts), 8), dtype=torch.int32, device="cuda:0")
    sd = ctx.signed_distance_device(src, attributes=True, out=(hits, attr))
    assert sd.hits.data_ptr() == hits.data_ptr() and sd.attr.data_ptr() == attr.data_ptr()
    torch.cuda.synchronize()
    want_sd = sd.hits.cpu().numpy().copy()
    assert np.array_equal(np.signbit(want_sd.view(np.float32)[:, 0]), (w3 & 1) == 1)
    # stream order: the points are made by a kernel behind a slow queue on a side stream, and overwritten right after the calls
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        a = slow_queue(torch, 12)
        p = (src + (a[0, 0] != a[0, 0]).to(torch.float32) * 0).contiguous()   # made behind the queue, on the side stream
        r1 = ctx.point_inside_device(p, counts=True, stream=side)
        r2 = ctx.point_inside_device(p, stream=side)
        r3 = ctx.signed_distance_device(p, stream=side)
        p.zero_()
        c1, c2, c3 = r1.count.clone(), r2.word.clone(), r3.hits.clone()
    side.synchronize()
    assert np.array_equal(c1.cpu().numpy().view(np.uint32), ref[:, :3]) and np.array_equal(c2.cpu().numpy().view(np.uint32), w3)
    assert np.array_equal(c3.cpu().numpy(), want_sd)
    # n == 0
    empty = torch.empty((0, 4), dtype=torch.float32, device="cuda:0")
    r = ctx.point_inside_device(empty, counts=True)
    assert r.word.shape == (0,) and r.count.shape == (0, 3) and r.inside.shape == (0,)
    r = ctx.signed_distance_device(empty, attributes=True)
    assert r.hits.shape == (0, 5) and r.attr.shape == (0, 8)
    hw, hc, _ = ctx.point_inside(np.zeros((0, 4), np.float32), counts=True)
    assert len(hw) == 0 and hc.shape == (0, 3)


@pytest.mark.gpu
def test_frame_in_flight_beside_an_inside_query():
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
        pts = small_points(sc, 400, seed=331)
        src = dev(pts)
        want = gpu_composed(base, pts, 3)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        slot.trace_async(W, H)
        with torch.cuda.stream(side):
            slow_queue(torch, 4)
            res = base.point_inside_device(src, counts=True, stream=side)
            sd = base.signed_distance_device(src, stream=side)
        during, _ = slot.trace_wait()
        after = base.trace(W, H)[0]
        side.synchronize()
        assert np.array_equal(during.view(np.uint32), before.view(np.uint32))
        assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
        w, cnt = res.numpy()
        assert cnt.tobytes() == want.tobytes() and np.array_equal(w, ir.words(cnt, 3, True)) and (cnt > 0).any()
        assert np.array_equal(np.signbit(sd.numpy()[0]["t"]), (w & 1) == 1)
    finally:
        slot.close()
        base.close()


def _raw(c, n, points, cull, n_dirs, words, counts):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_point_inside_device(c.h, n, p(points), cull, n_dirs, p(words), p(counts), None)


def _raw_sd(c, n, points, cull, n_dirs, hits, attr, words):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_signed_distance_device(c.h, n, p(points), cull, n_dirs, p(hits), p(attr), p(words), None)


@pytest.mark.gpu
def test_error_statuses():
    import torch
    from tests.test_blas_refit import span
    sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
    sc = cr.Scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances)
    p_np = small_points(sc, 100, seed=341)
    pt = dev(p_np)
    n = pt.shape[0]
    words = torch.empty((n + 1,), dtype=torch.int32, device="cuda:0")
    counts = torch.empty((5 * n + 1,), dtype=torch.int32, device="cuda:0")
    hits = torch.empty((n + 1, 5), dtype=torch.int32, device="cuda:0")
    attr = torch.empty((n + 1, 8), dtype=torch.int32, device="cuda:0")
    P_, W_, C_, H_, A_ = pt.data_ptr(), words.data_ptr(), counts.data_ptr(), hits.data_ptr(), attr.data_ptr()
    c = RtContext(0)
    ref = {}

    def err(fn, args, code, text):
        assert fn(c, *args) == code, args
        msg = c.L.rt_last_error(c.h).decode()
        assert text in msg, (args, msg)

    def ok():
        w, cnt = gpu_inside(c, p_np, 3, counts=True)
        if not ref:
            ref["cnt"] = gpu_composed(c, p_np, 3)
            assert (ref["cnt"] > 0).any()
        assert cnt.tobytes() == ref["cnt"].tobytes() and np.array_equal(w, ir.words(cnt, 3, True))

    try:
        err(_raw, (n, P_, 0xFF, 3, W_, 0), RT_ERR_NOT_READY, "")   # no geometry
        err(_raw_sd, (n, P_, 0xFF, 3, H_, 0, 0), RT_ERR_NOT_READY, "")
        c.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        err(_raw, (n, P_, 0xFF, 3, W_, 0), RT_ERR_NOT_READY, "")   # no TLAS
        err(_raw_sd, (n, P_, 0xFF, 3, H_, 0, 0), RT_ERR_NOT_READY, "")
        c.set_instances(sp.instances)
        c.set_uniforms(sp.uniforms)
        ok()
        bad = [((0xFFFFFF00, P_, 0xFF, 3, W_, 0), "too many points"), ((0x55555500, P_, 0xFF, 3, W_, C_), "n * n_dirs"),
               ((0x33333300, P_, 0xFF, 5, W_, C_), "n * n_dirs"), ((n, P_, 0x100, 3, W_, 0), "cull_mask"),
               ((n, P_, 0xFF, 0, W_, 0), "n_dirs"), ((n, P_, 0xFF, 2, W_, 0), "n_dirs"), ((n, P_, 0xFF, 4, W_, 0), "n_dirs"), ((n, P_, 0xFF, 7, W_, 0), "n_dirs"),
               ((n, 0, 0xFF, 3, W_, 0), "null point/word pointers"), ((n, P_, 0xFF, 3, 0, C_), "null point/word pointers"),
               ((n, P_ + 4, 0xFF, 3, W_, 0), "aligned"), ((n, P_, 0xFF, 3, W_ + 2, 0), "aligned"), ((n, P_, 0xFF, 3, W_, C_ + 1), "aligned")]
        bad_sd = [((0xFFFFFF00, P_, 0xFF, 3, H_, 0, 0), "too many points"), ((n, P_, 0x100, 3, H_, 0, 0), "cull_mask"), ((n, P_, 0xFF, 2, H_, 0, 0), "n_dirs"),
                  ((n, 0, 0xFF, 3, H_, 0, 0), "null point/hit pointers"), ((n, P_, 0xFF, 3, 0, 0, W_), "null point/hit pointers"),
                  ((n, P_ + 8, 0xFF, 3, H_, 0, 0), "aligned"), ((n, P_, 0xFF, 3, H_ + 2, 0, 0), "aligned"), ((n, P_, 0xFF, 3, H_, A_ + 4, 0), "aligned"),
                  ((n, P_, 0xFF, 3, H_, 0, W_ + 2), "aligned")]
        host_buf = np.zeros((n + 1, 8), np.float32)
        pinned = torch.zeros((n, 8), dtype=torch.float32).pin_memory()
        for ptr in ((host_buf.ctypes.data + 15) & ~15, pinned.data_ptr()):   # (16-byte aligned: only the memory kind is wrong)
            text = "device memory of the context's GPU"
            bad += [((n, ptr, 0xFF, 3, W_, 0), text), ((n, P_, 0xFF, 3, ptr, 0), text), ((n, P_, 0xFF, 3, W_, ptr), text)]
            bad_sd += [((n, ptr, 0xFF, 3, H_, 0, 0), text), ((n, P_, 0xFF, 3, ptr, 0, 0), text), ((n, P_, 0xFF, 3, H_, ptr, 0), text),
                       ((n, P_, 0xFF, 3, H_, 0, ptr), text)]
        for args, text in bad:
            err(_raw, args, RT_ERR_INVALID_ARGUMENT, text)
        ok()
        for args, text in bad_sd:
            err(_raw_sd, args, RT_ERR_INVALID_ARGUMENT, text)
        ok()
        # n * n_dirs is only bounded when the counts are asked for (refused later: no such memory is touched at these sizes)
        assert _raw(c, 0x55555500, P_, 0x100, 3, W_, 0) == RT_ERR_INVALID_ARGUMENT and "cull_mask" in c.L.rt_last_error(c.h).decode()
        # 4-byte aligned words and counts that are not 16-byte aligned are fine
        assert _raw(c, n, P_, 0xFF, 3, W_ + 4, C_ + 4) == 0
        torch.cuda.synchronize()
        assert counts[1:1 + 3 * n].cpu().numpy().tobytes() == ref["cnt"].tobytes()
        w = np.zeros(n, np.uint32); cn = np.zeros((n, 3), np.uint32)
        P = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        assert c.L.rt_point_inside(c.h, n, None, 0xFF, 3, P(w), None, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_point_inside(c.h, n, P(p_np), 0xFF, 3, None, P(cn), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_point_inside(c.h, n, P(p_np), 0x100, 3, P(w), None, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_point_inside(c.h, n, P(p_np), 0xFF, 2, P(w), None, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_point_inside(c.h, 0xFFFFFF00, P(p_np), 0xFF, 3, P(w), None, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_point_inside(c.h, 0x55555500, P(p_np), 0xFF, 3, P(w), P(cn), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_point_inside(c.h, n, P(p_np), 0xFF, 3, P(w), P(cn), 0, None) == 0 and cn.tobytes() == ref["cnt"].tobytes()
        ok()
        assert _raw(c, 0, 0, 0xFF, 3, 0, 0) == 0 and _raw_sd(c, 0, 0, 0xFF, 3, 0, 0, 0) == 0   # n == 0 enqueues nothing and needs no pointers
        with pytest.raises(ValueError):
            c.point_inside_device(pt.cpu())
        with pytest.raises(ValueError):
            c.point_inside_device(torch.zeros((4, 8), dtype=torch.float32, device="cuda:0"))
        with pytest.raises(ValueError):
            c.point_inside_device(pt, n_dirs=2)
        with pytest.raises(ValueError):
            c.signed_distance_device(pt, n_dirs=4)
        with pytest.raises(ValueError):
            c.signed_distance_device(pt.cpu())
        for call in (c.point_inside_device, c.signed_distance_device):
            with pytest.raises(RtError) as e:
                call(pt, cull_mask=0x1FF)
            assert e.value.code == RT_ERR_INVALID_ARGUMENT
        ok()
        # not ready: a stale TLAS after a BLAS refit
        ff, nf = span(sp.geom, 1)
        v = torch.from_numpy(sp.geom.verts[ff:ff + nf].copy()).to("cuda:0")
        torch.cuda.synchronize()
        c.refit_blas_device(1, v)
        err(_raw, (n, P_, 0xFF, 3, W_, 0), RT_ERR_NOT_READY, "")
        err(_raw_sd, (n, P_, 0xFF, 3, H_, 0, 0), RT_ERR_NOT_READY, "")
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
        err(_raw, (n, P_, 0xFF, 3, W_, 0), RT_ERR_INVALID_ARGUMENT, "trace_variant 0")
        err(_raw_sd, (n, P_, 0xFF, 3, H_, 0, 0), RT_ERR_INVALID_ARGUMENT, "trace_variant 0")
        a.set_param("trace_variant", 0)
        a.set_instances(sp.instances)
        ok()
    finally:
        a.close()


@pytest.mark.gpu
def test_cfg3_large(ctx):
    """1 << 18 points in cfg3's bounding box, GPU against GPU: the counts equal the all-hits count query of the 3 << 18 composed rays,
    the words the restated vote, and the early stop takes two directions for most points"""
    wl = workloads.make("cfg3", os.path.join(ROOT, "resources"), mesh="standin")
    wl.apply(ctx)
    g = wl.geometry
    sc = cr.Scene(g.verts, g.idx, g.ranges, wl.instances)
    lo, hi = scene_box(sc)
    rng = np.random.default_rng(351)
    n = 1 << 18
    pts = np.concatenate([lo + rng.uniform(size=(n, 3)) * (hi - lo), np.ones((n, 1))], axis=1).astype(np.float32)
    w, cnt = check(ctx, pts, 3, None, "cfg3")
    assert (cnt > 0).any() and (w & 1).any() and ((w >> 16) == 2).mean() > 0.5
    print("cfg3: %.3f of the points inside, %.3f decided after two directions" % ((w & 1).mean(), ((w >> 16) == 2).mean()))
