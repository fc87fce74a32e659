"""rt_intersect_device_flags: ray queries with rayQueryInitializeEXT's rayFlags and cullMask, for a whole call and per ray.

Most checks are bit-for-bit equivalences with rt_intersect_device, which tests/test_ray_query.py verifies against rt_intersect and the
oracle: neutral flags change nothing, a cull mask equals the plain query on instances whose masks were restricted beforehand, opacity
culls equal the plain query over the complementary instance set, and facing culls equal peeling (re-querying behind every culled hit)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import scenes
from tests.test_ray_query import PATHS, _resource_usage, check_attributes, dev, dev_inst, field, field_rays, mixed_rays, slow_queue
from vulkan_raytracing_amd import RtContext, api, host
from vulkan_raytracing_amd.api import HIT_DTYPE, RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
OPAQUE, NO_OPAQUE, TERMINATE = api.RAY_FLAG_OPAQUE, api.RAY_FLAG_NO_OPAQUE, api.RAY_FLAG_TERMINATE_ON_FIRST_HIT
CULL_BACK, CULL_FRONT = api.RAY_FLAG_CULL_BACK_FACING, api.RAY_FLAG_CULL_FRONT_FACING
CULL_OPAQUE, CULL_NO_OPAQUE, SKIP_TRIANGLES = api.RAY_FLAG_CULL_OPAQUE, api.RAY_FLAG_CULL_NO_OPAQUE, api.RAY_FLAG_SKIP_TRIANGLES
FCD, FLIP = api.INSTANCE_FLAG_FACING_CULL_DISABLE, api.INSTANCE_FLAG_FLIP_FACING
FORCE_OPAQUE, FORCE_NO_OPAQUE = api.INSTANCE_FLAG_FORCE_OPAQUE, api.INSTANCE_FLAG_FORCE_NO_OPAQUE
FRONT, BACK = 0xFE, 0xFF


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_header_declares_and_library_exports_intersect_device_flags():
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^int rt_intersect_device_flags\(rt_ctx\* ctx, size_t n, const void\* d_rays8, const void\* d_ray_words,\s*uint32_t ray_flags, "
                     r"uint32_t cull_mask,\s*void\* d_hits, void\* d_attr, void\* hip_stream\);", hdr, re.M)
    want = {"RT_RAY_FLAG_OPAQUE": 0x1, "RT_RAY_FLAG_NO_OPAQUE": 0x2, "RT_RAY_FLAG_TERMINATE_ON_FIRST_HIT": 0x4, "RT_RAY_FLAG_SKIP_CLOSEST_HIT": 0x8,
            "RT_RAY_FLAG_CULL_BACK_FACING": 0x10, "RT_RAY_FLAG_CULL_FRONT_FACING": 0x20, "RT_RAY_FLAG_CULL_OPAQUE": 0x40,
            "RT_RAY_FLAG_CULL_NO_OPAQUE": 0x80, "RT_RAY_FLAG_SKIP_TRIANGLES": 0x100, "RT_RAY_FLAG_SKIP_AABBS": 0x200,
            "RT_INSTANCE_FLAG_FACING_CULL_DISABLE": 0x1, "RT_INSTANCE_FLAG_FLIP_FACING": 0x2, "RT_INSTANCE_FLAG_FORCE_OPAQUE": 0x4,
            "RT_INSTANCE_FLAG_FORCE_NO_OPAQUE": 0x8}
    for name, v in want.items():
        m = re.search(r"^#define %s\s+(0x[0-9A-Fa-f]+)u" % name, hdr, re.M)
        assert m and int(m.group(1), 16) == v, name
        assert getattr(api, name[3:]) == v, name
    assert "rt_intersect_device_flags" in api.EXPORTS
    L = api.lib()
    assert hasattr(L, "rt_intersect_device_flags")
    assert L.rt_abi_version() == 7
    assert hasattr(RtContext, "intersect_device_flags")


def test_null_context_is_rejected_without_a_device():
    L = api.lib()
    assert L.rt_intersect_device_flags(None, 0, None, None, 0, 0xFF, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_intersect_device_flags(None, 64, None, None, CULL_BACK, 3, None, None, None) == RT_ERR_INVALID_ARGUMENT


# k_trace<MODE_QUERY_FLAGS = 4, ANY = 0, WIDE = 0, ENTRY = 0, FAR = 1, CONT = 0>
K_FLAGS = "_ZN2rt7k_traceILi4ELb0ELb0ELb0ELb1ELb0EEEvNS_9TraceArgsE"


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_flag_kernels_keep_their_budget(target):
    kernels = _resource_usage(target)
    assert K_FLAGS in kernels, "\n".join(kernels)
    r = kernels[K_FLAGS]
    assert int(r["Occupancy"]) >= 4 and int(r["ScratchSize"]) <= 32 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r
    kinds = [k for k in kernels if "k_hit_kind" in k]
    assert len(kinds) == 1, "\n".join(kernels)
    r = kernels[kinds[0]]
    assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, r


# ---- GPU helpers --------------------------------------------------------------------------------------------------------------

def qf(ctx, rays, flags=0, cull=0xFF, words=None, attributes=False):
    """a flag-aware device query of host rays, collected after a device synchronisation: (hits, attributes or None)"""
    import torch
    t = rays if isinstance(rays, torch.Tensor) else dev(rays)
    w = None if words is None else torch.from_numpy(np.ascontiguousarray(words, np.uint32).view(np.int32).copy()).to("cuda:0")
    res = ctx.intersect_device_flags(t, ray_flags=flags, cull_mask=cull, words=w, attributes=attributes)
    torch.cuda.synchronize()
    return res.numpy()


def q(ctx, rays, any_hit=False, attributes=False):
    import torch
    res = ctx.intersect_device(dev(rays), any_hit=any_hit, attributes=attributes)
    torch.cuda.synchronize()
    return res.numpy()


def field_scene(ctx, inst):
    geom = host.SceneGeometry(PATHS)
    u = host.default_uniforms(max_bounce_count=2, samples_per_pixel=1, center_object_type=1, orbiting_object_type=0,
                              orbiting_object_primitive_offset=geom.orbiting_primitive_offset, orbiting_object_vertex_offset=geom.orbiting_vertex_offset)
    return scenes.ScenePair(PATHS, inst, u, ctx=ctx), geom


def with_flags(inst, flags):
    out = inst.copy()
    out["sbt_offset_and_flags"] = (np.asarray(flags, np.uint32) & 0xFF) << 24
    return out


def with_masks(inst, masks):
    out = inst.copy()
    out["custom_index_and_mask"] = (out["custom_index_and_mask"] & 0xFFFFFF) | ((np.asarray(masks, np.uint32) & 0xFF) << 24)
    return out


def check_kinds(attr, hits):
    k = attr[:, 7]
    hit = hits["inst"] >= 0
    assert np.isin(k[hit], [FRONT, BACK]).all() and (k[~hit] == 0).all()


@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


# ---- 1. neutral flags ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["teapot_cube", "field"])
def test_neutral_flags_equal_intersect_device(ctx, scene):
    if scene == "teapot_cube":
        sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=ctx)
        rays = mixed_rays(20_000, seed=31)
    else:
        sp, _ = field_scene(ctx, field(500, seed=32))
        rays = np.concatenate([field_rays(40_000, seed=33), mixed_rays(2000, seed=34)])
    n = len(rays)
    closest, ca = q(ctx, rays, attributes=True)
    anyh, _ = q(ctx, rays, any_hit=True)
    assert (closest["inst"] >= 0).mean() > 0.05
    for flags in (0, OPAQUE, api.RAY_FLAG_SKIP_CLOSEST_HIT, api.RAY_FLAG_SKIP_AABBS):
        for words in (None, np.full(n, 0xFF000000, np.uint32)):
            h, a = qf(ctx, rays, flags, 0xFF, words, attributes=True)
            assert h.tobytes() == closest.tobytes(), (flags, words is None)
            assert np.array_equal(a[:, :7], ca[:, :7])
            check_kinds(a, h)
    h, a = qf(ctx, rays, TERMINATE, attributes=True)
    assert h.tobytes() == anyh.tobytes()
    check_attributes(np.concatenate([a[:, :7], np.zeros((n, 1), np.int32)], axis=1), h, sp.orc)   # (word 7: the hit kind)
    # a per-ray mix: ray for ray the matching query
    rng = np.random.default_rng(35)
    term = rng.random(n) < 0.5
    words = np.where(term, 0xFF000000 | TERMINATE, 0xFF000000).astype(np.uint32)
    h, _ = qf(ctx, rays, 0, 0xFF, words)
    assert h[term].tobytes() == anyh[term].tobytes() and h[~term].tobytes() == closest[~term].tobytes()
    # bits 10-23 of a word are ignored
    h, _ = qf(ctx, rays, 0, 0xFF, words | 0x00FFFC00)
    assert h[term].tobytes() == anyh[term].tobytes() and h[~term].tobytes() == closest[~term].tobytes()


# ---- 2. cull mask -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("records", ["host", "device"])
def test_cull_mask_equals_restricted_instances(ctx, records):
    import torch
    inst = field(400, seed=41)
    masks = np.array([(1 << (i % 8)) if i % 11 else (0xFF if i % 2 else 0) for i in range(len(inst))], np.uint32)
    inst = with_masks(inst, masks)
    field_scene(ctx, inst)
    rays = field_rays(30_000, seed=42)

    def use(records_inst):
        if records == "host":
            ctx.set_instances(records_inst)
        else:
            torch.cuda.synchronize()
            ctx.set_instances_device(dev_inst(records_inst))

    refs = {}
    for M in (0xFF, 0x01, 0x0A, 0x80, 0x00):
        use(with_masks(inst, masks & M))
        refs[M], _ = q(ctx, rays)
    use(inst)
    for M, ref in refs.items():
        h, _ = qf(ctx, rays, 0, M)
        assert h.tobytes() == ref.tobytes(), M
    assert (refs[0x00]["inst"] < 0).all() and refs[0x01].tobytes() != refs[0xFF].tobytes()
    # per-ray cull masks equal the query grouped by mask (and combine with the call's mask by AND)
    rng = np.random.default_rng(43)
    ms = np.array(list(refs), np.uint32)[rng.integers(0, len(refs), len(rays))]
    h, _ = qf(ctx, rays, 0, 0xFF, ms << 24)
    for M, ref in refs.items():
        sel = ms == M
        assert h[sel].tobytes() == ref[sel].tobytes(), M
    h, _ = qf(ctx, rays, 0, 0x0B, np.full(len(rays), 0x0E000000, np.uint32))
    assert h.tobytes() == refs[0x0A].tobytes()


# ---- 3. facing ----------------------------------------------------------------------------------------------------------------

def one_triangle(ctx, flags):
    """one triangle (0,0,0), (1,0,0), (0,1,0) in z = 0 under the identity: counter-clockwise seen from +z"""
    v = np.array([[0, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 1], [0, 1, 0, 0, 0, 1]], np.float32).reshape(-1)
    ctx.upload_geometry(v, np.array([0, 1, 2], np.uint32), [(0, 0, 1)])
    t = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    inst = with_flags(np.array([host.make_instance(t, 0, 0)]), flags)
    ctx.set_instances(inst)


@pytest.mark.gpu
def test_facing_convention_on_one_triangle():
    """front-facing <=> det < 0: the triangle is counter-clockwise seen from +z, so a ray from +z looking down sees its back face"""
    c = RtContext(0)
    try:
        from_above = [0.25, 0.25, 5.0, 0.0, 0, 0, -1, 100.0]
        from_below = [0.25, 0.25, -5.0, 0.0, 0, 0, 1, 100.0]
        rays = np.array([from_above, from_below], np.float32)
        for iflags, kinds in ((0, (BACK, FRONT)), (FLIP, (FRONT, BACK)), (FCD, (BACK, FRONT)), (FCD | FLIP, (FRONT, BACK))):
            one_triangle(c, iflags)
            h, a = qf(c, rays, 0, attributes=True)
            assert (h["inst"] == 0).all() and (h["t"] == 5.0).all()
            assert tuple(a[:, 7]) == kinds, iflags
            for cull, culled in ((CULL_BACK, BACK), (CULL_FRONT, FRONT)):
                h, a = qf(c, rays, cull, attributes=True)
                gone = np.array(kinds) == culled
                if iflags & FCD:
                    gone[:] = False
                assert ((h["inst"] < 0) == gone).all(), (iflags, cull)
                assert (a[~gone, 7] == np.array(kinds)[~gone]).all()
                for w in (cull, cull | TERMINATE):   # the same through the ray words
                    h2, _ = qf(c, rays, 0, 0xFF, np.full(2, 0xFF000000 | w, np.uint32))
                    assert h2.tobytes() == h.tobytes()
    finally:
        c.close()


def object_det(inst, geom, hits, rays):
    """float64 det = dot(e1, cross(d_obj, e2)) of each hit, and its relative size"""
    det = np.zeros(len(hits)); rel = np.zeros(len(hits))
    for k in np.nonzero(hits["inst"] >= 0)[0]:
        I = inst[hits["inst"][k]]
        M = I["transform"].astype(np.float64).reshape(3, 4)[:, :3]
        ff, fi, _ = geom.ranges[int(I["mesh"])]
        ix = geom.idx[fi + 3 * hits["prim"][k]: fi + 3 * hits["prim"][k] + 3]
        p = [geom.verts[ff + 6 * int(j): ff + 6 * int(j) + 3].astype(np.float64) for j in ix]
        e1, e2 = p[1] - p[0], p[2] - p[0]
        d = np.linalg.solve(M, rays[k, 4:7].astype(np.float64))
        det[k] = np.dot(e1, np.cross(d, e2))
        rel[k] = abs(det[k]) / (np.linalg.norm(e1) * np.linalg.norm(e2) * np.linalg.norm(d) + 1e-300)
    return det, rel


@pytest.mark.gpu
def test_facing_culls_equal_peeling(ctx):
    inst = field(300, seed=51)
    iflags = np.array([[0, FLIP, FCD, 0, FLIP | FCD][i % 5] for i in range(len(inst))], np.uint32)
    inst = with_flags(inst, iflags)
    _, geom = field_scene(ctx, inst)
    rays = field_rays(6000, seed=52)
    n = len(rays)
    for cull in (CULL_BACK, CULL_FRONT):
        h, a = qf(ctx, rays, cull, attributes=True)
        # the reported hit kind is never the culled one (on instances that do not disable culling)
        fl = iflags[np.maximum(h["inst"], 0)]
        live = (h["inst"] >= 0) & ((fl & FCD) == 0)
        assert not (a[live, 7] == (BACK if cull == CULL_BACK else FRONT)).any()
        # peel with rt_intersect_device
        cur = rays.copy()
        want = np.zeros(n, HIT_DTYPE); want["inst"] = -1; want["prim"] = -1
        done = np.zeros(n, bool); bad = np.zeros(n, bool)
        seen = [set() for _ in range(n)]
        for _ in range(64):
            act = np.nonzero(~done)[0]
            if len(act) == 0:
                break
            g, _ = q(ctx, cur[act])
            det, rel = object_det(inst, geom, g, cur[act])
            for j, k in enumerate(act):
                if g["inst"][j] < 0:
                    want[k] = g[j]; done[k] = True; continue
                f = int(iflags[g["inst"][j]])
                front = (det[j] < 0) != bool(f & FLIP)
                if rel[j] < 1e-5 or float(g["t"][j]) in seen[k]:
                    bad[k] = True; done[k] = True; continue
                seen[k].add(float(g["t"][j]))
                culled = not (f & FCD) and ((cull == CULL_BACK and not front) or (cull == CULL_FRONT and front))
                if culled:
                    cur[k, 3] = g["t"][j]
                else:
                    want[k] = g[j]; done[k] = True
        ok = done & ~bad
        assert bad.sum() < 0.02 * n and ok.sum() > 0.9 * n, (bad.sum(), ok.sum())
        assert h[ok].tobytes() == want[ok].tobytes(), cull
        assert (want["inst"][ok] >= 0).mean() > 0.02
    # instances with FACING_CULL_DISABLE ignore facing culls
    all_fcd = with_flags(inst, iflags | FCD)
    ctx.set_instances(all_fcd)
    ref, _ = q(ctx, rays)
    for cull in (CULL_BACK, CULL_FRONT):
        h, _ = qf(ctx, rays, cull)
        assert h.tobytes() == ref.tobytes()


# ---- 4. opacity ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_opacity(ctx):
    inst = field(300, seed=61)
    _, geom = field_scene(ctx, inst)
    rays = field_rays(20_000, seed=62)
    full, _ = q(ctx, rays)
    assert (full["inst"] >= 0).mean() > 0.02
    for flags in (SKIP_TRIANGLES, CULL_OPAQUE):
        h, _ = qf(ctx, rays, flags)
        assert (h["inst"] < 0).all(), flags
    h, _ = qf(ctx, rays, CULL_NO_OPAQUE)
    assert h.tobytes() == full.tobytes()
    # FORCE_NO_OPAQUE on every third instance: CullOpaque sees only those, CullNoOpaque only the others
    nopq = np.arange(len(inst)) % 3 == 0
    flagged = with_flags(inst, np.where(nopq, FORCE_NO_OPAQUE | FCD, FCD))
    orig_masks = inst["custom_index_and_mask"] >> 24
    ctx.set_instances(with_masks(flagged, np.where(nopq, orig_masks, 0)))
    only_nopq, _ = q(ctx, rays)
    ctx.set_instances(with_masks(flagged, np.where(nopq, 0, orig_masks)))
    only_opq, _ = q(ctx, rays)
    ctx.set_instances(flagged)
    assert qf(ctx, rays, CULL_OPAQUE)[0].tobytes() == only_nopq.tobytes()
    assert qf(ctx, rays, CULL_NO_OPAQUE)[0].tobytes() == only_opq.tobytes()
    # the ray's OPAQUE overrides FORCE_NO_OPAQUE (per ray too), NO_OPAQUE overrides the default
    assert qf(ctx, rays, 0, 0xFF, np.full(len(rays), 0xFF000000 | OPAQUE | CULL_NO_OPAQUE, np.uint32))[0].tobytes() == full.tobytes()
    assert (qf(ctx, rays, 0, 0xFF, np.full(len(rays), 0xFF000000 | NO_OPAQUE | CULL_NO_OPAQUE, np.uint32))[0]["inst"] < 0).all()
    assert qf(ctx, rays, NO_OPAQUE)[0].tobytes() == full.tobytes()
    # FORCE_OPAQUE wins over the default: everything is opaque again
    ctx.set_instances(with_flags(inst, np.where(nopq, FORCE_OPAQUE | FCD, FCD)))
    assert (qf(ctx, rays, CULL_OPAQUE)[0]["inst"] < 0).all()


# ---- 5. first hit with culling ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_first_hit_with_culling(ctx):
    inst = field(300, seed=71)
    iflags = np.array([[0, FLIP, FCD][i % 3] for i in range(len(inst))], np.uint32)
    inst = with_flags(inst, iflags)
    sp, geom = field_scene(ctx, inst)
    rays = field_rays(4000, seed=72)
    closest, _ = qf(ctx, rays, CULL_BACK)
    first, a = qf(ctx, rays, CULL_BACK | TERMINATE, attributes=True)
    assert np.array_equal(first["inst"] < 0, closest["inst"] < 0)
    hit = first["inst"] >= 0
    assert hit.mean() > 0.02
    # every reported hit lies on the ray (some element of its full peel sequence: re-query closest hit from just before it)
    probe = rays.copy()
    probe[hit, 3] = np.nextafter(first["t"][hit], np.float32(-np.inf))
    g, _ = q(ctx, probe)
    assert (g["t"][hit] == first["t"][hit]).all()
    # ... and is not culled
    det, rel = object_det(inst, geom, first, rays)
    front = (det < 0) != ((iflags[np.maximum(first["inst"], 0)] & FLIP) != 0)
    sure = hit & (rel >= 1e-5) & ((iflags[np.maximum(first["inst"], 0)] & FCD) == 0)
    assert front[sure].all()
    check_attributes(np.concatenate([a[:, :7], np.zeros((len(rays), 1), np.int32)], axis=1), first, sp.orc)
    check_kinds(a, first)


# ---- 6. stream order ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_words_are_read_in_stream_order(ctx):
    import torch
    inst = field(200, seed=81)
    field_scene(ctx, inst)
    rays_np = field_rays(30_000, seed=82)
    ref, _ = q(ctx, rays_np, any_hit=True)
    rays = dev(rays_np)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = slow_queue(torch)
        words = torch.full((len(rays_np),), 0x7F000000, dtype=torch.int32, device="cuda:0")
        words += ((a[0, 0] == a[0, 0]).to(torch.int32) * (TERMINATE - 0x7F000000 - 0x1000000))   # -> 0xFF000000 | TERMINATE, behind the queue
        res = ctx.intersect_device_flags(rays, words=words, attributes=True, stream=s)
        words.zero_()
        hits = res.hits.clone()
    s.synchronize()
    assert hits.cpu().numpy().view(HIT_DTYPE).reshape(-1).tobytes() == ref.tobytes()


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------

def _raw(c, n, rays, words, flags, cull, hits, attr=0):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_intersect_device_flags(c.h, n, p(rays), p(words), flags, cull, p(hits), p(attr), None)


@pytest.mark.gpu
def test_error_statuses():
    import torch
    rays_np = mixed_rays(1000, seed=90)
    rays = dev(rays_np)
    n = rays.shape[0]
    hits = torch.empty((n, 5), dtype=torch.int32, device="cuda:0")
    words = torch.full((n + 1,), -16777216, dtype=torch.int32, device="cuda:0")
    R_, H_, W_ = rays.data_ptr(), hits.data_ptr(), words.data_ptr()
    c = RtContext(0)
    try:
        assert _raw(c, n, R_, 0, 0, 0xFF, H_) == RT_ERR_NOT_READY
        sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
        c.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        assert _raw(c, n, R_, 0, 0, 0xFF, H_) == RT_ERR_NOT_READY
        c.set_instances(sp.instances)
        ref, _ = q(c, rays_np)
        bad_flags = [(0x400, 0xFF), (0, 0x100), (OPAQUE | NO_OPAQUE, 0xFF), (OPAQUE | CULL_OPAQUE, 0xFF), (CULL_OPAQUE | CULL_NO_OPAQUE, 0xFF),
                     (NO_OPAQUE | CULL_NO_OPAQUE, 0xFF), (CULL_BACK | CULL_FRONT, 0xFF), (SKIP_TRIANGLES | api.RAY_FLAG_SKIP_AABBS, 0xFF),
                     (SKIP_TRIANGLES | CULL_BACK, 0xFF), (SKIP_TRIANGLES | CULL_FRONT, 0xFF)]
        for flags, cull in bad_flags:
            assert _raw(c, n, R_, W_, flags, cull, H_) == RT_ERR_INVALID_ARGUMENT, (flags, cull)
            assert c.L.rt_last_error(c.h)
        host_words = np.zeros(n, np.uint32)
        for w in (W_ + 2, host_words.ctypes.data):   # misaligned, host memory
            assert _raw(c, n, R_, w, 0, 0xFF, H_) == RT_ERR_INVALID_ARGUMENT
        assert _raw(c, n, R_ + 4, W_, 0, 0xFF, H_) == RT_ERR_INVALID_ARGUMENT
        assert _raw(c, n, R_, W_, 0, 0xFF, 0) == RT_ERR_INVALID_ARGUMENT
        assert _raw(c, 0, 0, 0, 0, 0xFF, 0) == 0
        with pytest.raises(RtError) as e:
            c.intersect_device_flags(rays, ray_flags=CULL_BACK | CULL_FRONT)
        assert e.value.code == RT_ERR_INVALID_ARGUMENT
        with pytest.raises(ValueError):
            c.intersect_device_flags(rays, words=words[:n].cpu())
        assert qf(c, rays_np, SKIP_TRIANGLES | OPAQUE)[0]["inst"].max() == -1   # a valid combination
        assert qf(c, rays_np)[0].tobytes() == ref.tobytes()
        c.set_batch(np.stack([sp.instances, sp.instances]), np.stack([sp.uniforms, sp.uniforms]).reshape(-1))
        assert _raw(c, n, R_, W_, 0, 0xFF, H_) == RT_ERR_NOT_READY
        c.set_instances(sp.instances)
        assert qf(c, rays_np)[0].tobytes() == ref.tobytes()
    finally:
        c.close()


# ---- 8. frames ignore instance flags ------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_frames_ignore_instance_flags():
    c = RtContext(0)
    try:
        sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, sky=scenes.synthetic_skybox(64), ctx=c)
        W, H = 400, 224
        ref, _ = c.trace(W, H)
        c.set_instances(with_flags(sp.instances, FLIP | FORCE_NO_OPAQUE))
        img, _ = c.trace(W, H)
        assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
        # ... while the same records reach ray queries: FORCE_NO_OPAQUE everywhere, so CullNoOpaque hides everything
        rays = mixed_rays(2000, seed=91)
        assert (qf(c, rays)[0]["inst"] >= 0).any()
        assert (qf(c, rays, CULL_NO_OPAQUE)[0]["inst"] < 0).all()
    finally:
        c.close()
