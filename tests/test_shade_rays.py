"""rt_shade_rays_device: the frame's bounce pipeline on caller-generated primary rays in device memory (custom ray generation).

The colours must be those of the reference's bounce loop (src/shader.rgen:84-177) for the same rays: per sample against a reference
composed from the oracle's own exports (tests/shade_reference.py), per point against the frame itself for the pinhole rays of a frame
(bit for bit).  The ordering tests check that the call reads its rays, TLAS and scene in stream order and that nothing the library does
afterwards changes what it returns."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import oracle
from tests import scenes
from tests.shade_reference import AMBIENT, average_points, pinhole_rays, shade_samples
from vulkan_raytracing_amd import RtContext, api, host, workloads
from vulkan_raytracing_amd.api import INSTANCE_DTYPE, MATERIAL_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = scenes.RES
TEAPOT, CUBE = os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj")
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2


def mixed_scene(max_bounce, spp, ctx=None, sky=True):
    """cfg2-style mixed scene: the refractive teapot at M0, the diffuse cube orbiting at M1, and a mirror cube (mesh 1, scaled 2) off
    to the side; instance types (2, 0, 1)"""
    inst = list(host.SceneAnimation().instances((0, 1)))
    inst.append(host.make_instance(np.array([2, 0, 0, -5, 0, 2, 0, 0.5, 0, 0, 2, -3], np.float32), 1, 1))
    g = host.SceneGeometry([TEAPOT, CUBE])
    u = host.default_uniforms(max_bounce_count=max_bounce, samples_per_pixel=spp, center_object_type=2, orbiting_object_type=0,
                              orbiting_object_primitive_offset=g.orbiting_primitive_offset, orbiting_object_vertex_offset=g.orbiting_vertex_offset)
    sp = scenes.ScenePair([TEAPOT, CUBE], np.asarray(inst, INSTANCE_DTYPE), u, sky=scenes.synthetic_skybox(64) if sky else None, ctx=ctx)
    sp.set_instance_types(np.array([2, 0, 1], np.uint32))
    return sp


def material_table(sp):
    n_prims = len(sp.geom.idx) // 3
    table = np.zeros(4, MATERIAL_DTYPE)
    table[0] = ((0.1, 0.2, 0.3), 12.0, (0.9, 0.3, 0.5), 1.3, (0.2, 0.2, 0.2), api.MATERIAL_TYPE_OF_INSTANCE)
    table[1] = ((0.3, 0.1, 0.1), 50.0, (0.3, 0.8, 0.5), 1.5, (0.6, 0.6, 0.6), 0)
    table[2] = ((0.2, 0.2, 0.2), 10.0, (0.5, 0.5, 0.5), 1.7, (0.2, 0.2, 0.2), 1)
    table[3] = ((0.05, 0.3, 0.2), 3.0, (0.1, 0.9, 0.9), 1.1, (0.9, 0.9, 0.9), 2)
    pm = ((np.arange(n_prims) * 7 // 5) % 4).astype(np.uint32)
    return table, pm


def fisheye_rays(n_side, position=(0.0, 1.5, 14.0), tmax=10000.0):
    """an equidistant 180-degree fisheye looking down -z: the points of an n_side x n_side grid inside the unit circle"""
    v, u = np.mgrid[0:n_side, 0:n_side]
    u = (u + 0.5) / n_side * 2.0 - 1.0
    v = 1.0 - (v + 0.5) / n_side * 2.0
    r = np.hypot(u, v)
    keep = r <= 1.0
    u, v, r = u[keep], v[keep], r[keep]
    th, ph = r * (np.pi / 2), np.arctan2(v, u)
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((len(d), 8), np.float32)
    rays[:, 0:3] = position; rays[:, 4:7] = d; rays[:, 7] = tmax
    return rays


def inside_rays(geom, n, seed):
    """rays that start inside the teapot (mesh 0 at the origin): origins near the centre of its box, random directions"""
    v = np.asarray(geom.verts, np.float32).reshape(-1, 6)[:, 0:3]
    lo, hi = v.min(0), v.max(0)
    c, e = (lo + hi) / 2, (hi - lo) / 2
    rng = np.random.default_rng(seed)
    o = c + rng.uniform(-0.15, 0.15, (n, 3)) * e
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = o; rays[:, 4:7] = d; rays[:, 7] = 10000.0
    return rays


def arbitrary_rays(sp, seed):
    """random rays, rays from inside the refractive teapot, fisheye rays; a third of them with a random tmax in [0.0005, 10000]"""
    rays = np.concatenate([scenes.random_rays(3000, seed=seed), inside_rays(sp.geom, 600, seed + 1), fisheye_rays(48)])
    rng = np.random.default_rng(seed + 2)
    pick = rng.random(len(rays)) < 1 / 3
    rays[pick, 7] = (10.0 ** rng.uniform(np.log10(0.0005), 4.0, pick.sum())).astype(np.float32)
    rays[:, 3] = rng.uniform(-5, 5, len(rays)).astype(np.float32)   # word 3 is ignored
    return rays


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_abi_exports_shade_rays_device():
    assert "rt_shade_rays_device" in api.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^int rt_shade_rays_device\(rt_ctx\* ctx, size_t n_points, uint32_t n_samples, const void\* d_rays8, void\* d_sample_rgba, "
                     r"void\* d_point_rgba, void\* hip_stream\);", hdr, re.M)
    L = api.lib()
    assert hasattr(L, "rt_shade_rays_device")
    assert L.rt_abi_version() == 7
    assert hasattr(RtContext, "shade_rays_device")
    assert L.rt_shade_rays_device(None, 0, 1, None, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_shade_rays_device(None, 64, 4, None, None, None, None) == RT_ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_shade_kernels_use_no_scratch(target):
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    found = set()
    for name, r in kernels.items():
        for k in ("k_ray_ingest", "k_resolve_points"):
            if k in name:
                found.add(k)
                assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
    assert found == {"k_ray_ingest", "k_resolve_points"}


def test_composed_reference_equals_the_oracle_frame():
    """the yardstick: the composed reference on the pinhole rays of a frame is orc.render_pixels bit for bit (mixed types, depth 4,
    spp 4), with and without a material table"""
    W, H, spp, mb = 20, 14, 4, 4
    sp = mixed_scene(mb, spp)
    xy = np.stack(np.meshgrid(np.arange(W), np.arange(H)), -1).reshape(-1, 2)
    rays = pinhole_rays(sp.orc, W, H, spp)
    for mats in (None, material_table(sp)):
        if mats is not None:
            sp.set_materials(*mats)
        ref = sp.orc.render_pixels(W, H, xy)
        s = shade_samples(sp.orc, rays, W * H, mb, sp.instances, sp.geom.ranges, mats)
        pts = average_points(s, W * H, spp)
        assert np.array_equal(pts.view(np.uint32), ref.view(np.uint32)), mats is not None
        assert (s[:, 3] == 1).all()
        # (most samples are not the ambient term)
        assert (s[:, 0:3] != AMBIENT).any(1).mean() > 0.5


# ---- GPU helpers --------------------------------------------------------------------------------------------------------------

def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1, 8).copy()).to("cuda:0")


def shade(ctx, rays, samples=1, stream=None, **kw):
    import torch
    t = rays if isinstance(rays, torch.Tensor) else dev(rays)
    s, p = ctx.shade_rays_device(t, samples=samples, stream=stream, **kw)
    torch.cuda.synchronize()
    return (s.cpu().numpy() if s is not None else None), (p.cpu().numpy() if p is not None else None)


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


def check_pinhole(ctx, orc, W, H, spp):
    rays = pinhole_rays(orc, W, H, spp)
    img, _ = ctx.trace(W, H)
    s, p = shade(ctx, rays, samples=spp)
    assert same(p, img.reshape(-1, 4))
    assert (s[:, 3] == 1).all()
    assert same(average_points(s, W * H, spp), p)
    # points only (the per-sample colours in the call's own buffer), and samples only
    _, p2 = shade(ctx, rays, samples=spp, per_sample=False)
    s2, _ = shade(ctx, rays, samples=spp, points=False)
    assert same(p2, p) and same(s2, s)
    return img


# ---- 4. pinhole parity with the frame -----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_pinhole_parity_cfg3(ctx):
    w = workloads.make("cfg3", RES)
    w.apply(ctx)
    orc = oracle.OracleScene()
    orc.set_uniforms(w.uniforms.tobytes())
    img = check_pinhole(ctx, orc, 192, 108, 4)
    assert (img[..., 0] != img[0, 0, 0]).mean() > 0.05


@pytest.mark.gpu
def test_pinhole_parity_mixed_types_depth6(ctx):
    sp = scenes.two_object_scene(TEAPOT, CUBE, 2, 1, 6, 4, sky=scenes.synthetic_skybox(64), ctx=ctx)
    check_pinhole(ctx, sp.orc, 192, 108, 4)
    sp = mixed_scene(6, 3, ctx=ctx)
    check_pinhole(ctx, sp.orc, 160, 90, 3)


@pytest.mark.gpu
def test_pinhole_parity_materials_and_instance_types(ctx):
    sp = mixed_scene(5, 4, ctx=ctx)
    sp.set_materials(*material_table(sp))
    try:
        check_pinhole(ctx, sp.orc, 192, 108, 4)
    finally:
        ctx.set_materials(None)


@pytest.mark.gpu
def test_pinhole_parity_far_camera(ctx):
    """a camera 800 units from the scene (far rays: the quantised boxes need the far-ray logic)"""
    sp = mixed_scene(3, 2, ctx=ctx)
    u = sp.uniforms.copy()
    u[0]["position"][:3] = (0.0, 0.5, 800.0)
    sp.set_uniforms(u)
    img = check_pinhole(ctx, sp.orc, 192, 108, 2)
    # the scene covers a few pixels from there
    r = pinhole_rays(sp.orc, 192, 108, 1)
    assert (sp.orc.intersect(r)["inst"] >= 0).sum() > 0
    assert img.shape == (108, 192, 4)


# ---- 5. arbitrary rays against the composed reference -------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("max_bounce", [0, 1, 6, 63])
def test_arbitrary_rays_equal_the_reference(ctx, max_bounce):
    sp = mixed_scene(max_bounce, 1, ctx=ctx)
    rays = arbitrary_rays(sp, seed=40 + max_bounce)
    for samples in (1, 3):
        r = rays[:len(rays) // samples * samples]
        n_points = len(r) // samples
        ref = shade_samples(sp.orc, r, n_points, max_bounce)
        s, p = shade(ctx, r, samples=samples)
        bad = np.nonzero((s.view(np.uint32) != ref.view(np.uint32)).any(1))[0]
        assert len(bad) == 0, (samples, bad[:10], s[bad[:3]], ref[bad[:3]], r[bad[:3]])
        assert same(p, average_points(ref, n_points, samples))
    # the rays from inside the refractive teapot do start inside it
    ir = inside_rays(sp.geom, 600, 41 + max_bounce)
    ir[:, 3] = 0.001
    assert (sp.orc.intersect(ir)["inst"] == 0).mean() > 0.9


@pytest.mark.gpu
def test_arbitrary_rays_with_materials(ctx):
    sp = mixed_scene(6, 1, ctx=ctx)
    mats = material_table(sp)
    sp.set_materials(*mats)
    try:
        rays = arbitrary_rays(sp, seed=77)
        ref = shade_samples(sp.orc, rays, len(rays), 6, sp.instances, sp.geom.ranges, mats)
        s, _ = shade(ctx, rays, points=False)
        assert same(s, ref)
    finally:
        ctx.set_materials(None)


# ---- 6. invalid records -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_invalid_records(ctx):
    sp = mixed_scene(3, 1, ctx=ctx)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    good = scenes.random_rays(8, seed=5)
    bad = np.repeat(good[:1], 8, 0)
    bad[0, 0] = nan; bad[1, 2] = inf; bad[2, 4] = nan; bad[3, 6] = -inf; bad[4, 4:7] = 0.0; bad[5, 1] = -inf
    bad[6, 7] = 0.001; bad[7, 7] = 0.0005     # empty intervals: misses
    rays = np.concatenate([bad, good])         # 2 samples of 8 points: sample 0 the odd records, sample 1 good rays
    s, p = shade(ctx, rays, samples=2)
    assert (s[:6] == 0).all()
    for k in (6, 7):
        assert same(s[k, 0:3], sp.orc.sample_sky(np.array([bad[k, 4], bad[k, 5], -bad[k, 6]], np.float32))) and s[k, 3] == 1
    ref = shade_samples(sp.orc, rays, 8, 3)
    assert same(s, ref)
    assert same(p, average_points(ref, 8, 2))
    assert (p[:6, 3] == 0.5).all() and (p[6:, 3] == 1).all()


# ---- 7. argument errors -------------------------------------------------------------------------------------------------------

def _call(ctx, n_points, n_samples, rays, srgba, prgba, stream=None):
    ptr = lambda t: None if t is None else ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())
    return ctx.L.rt_shade_rays_device(ctx.h, n_points, n_samples, ptr(rays), ptr(srgba), ptr(prgba), stream)


@pytest.mark.gpu
def test_argument_errors(ctx):
    import torch
    sp = mixed_scene(2, 1, ctx=ctx)
    rays = dev(scenes.random_rays(64, seed=2))
    so = torch.empty((64, 4), dtype=torch.float32, device="cuda:0")
    po = torch.empty((64, 4), dtype=torch.float32, device="cuda:0")
    assert _call(ctx, 64, 1, rays, so, po) == 0
    torch.cuda.synchronize()
    E = RT_ERR_INVALID_ARGUMENT
    assert ctx.L.rt_shade_rays_device(None, 64, 1, ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(so.data_ptr()), None, None) == E
    assert _call(ctx, 64, 1, None, so, po) == E                        # NULL rays
    assert _call(ctx, 64, 1, rays, None, None) == E                    # no output
    assert _call(ctx, 0, 1, rays, None, None) == E
    assert _call(ctx, 16, 1, rays.data_ptr() + 4, so, None) == E       # misaligned
    assert _call(ctx, 16, 1, rays, so.data_ptr() + 8, None) == E
    assert _call(ctx, 16, 1, rays, None, po.data_ptr() + 4) == E
    host_buf = np.zeros((64, 4), np.float32)
    assert _call(ctx, 16, 1, rays, host_buf.ctypes.data, None) == E    # not device memory
    host_rays = np.zeros((64, 8), np.float32)
    assert _call(ctx, 16, 1, host_rays.ctypes.data, so, None) == E
    assert _call(ctx, 16, 0, rays, so, po) == E                        # n_samples == 0
    assert _call(ctx, (1 << 25) + 1, 1, rays, so, po) == E            # n > 2^25
    assert _call(ctx, 1 << 24, 3, rays, so, po) == E
    assert _call(ctx, 1 << 62, 4, rays, so, po) == E
    u = sp.uniforms.copy()
    u[0]["max_bounce_count"] = 70
    ctx.set_uniforms(u)
    assert _call(ctx, 16, 1, rays, so, po) == E                        # maxBounceCount above the frame limit (69)
    with pytest.raises(api.RtError) as e:
        ctx.trace(32, 16)
    assert e.value.code == E                                           # (the same limit as a frame's)
    u[0]["max_bounce_count"] = 69
    ctx.set_uniforms(u)
    assert _call(ctx, 16, 1, rays, so, po) == 0
    torch.cuda.synchronize()
    ctx.trace(32, 16)
    ctx.set_uniforms(sp.uniforms)
    with pytest.raises(ValueError):
        ctx.shade_rays_device(rays[:63], samples=2)
    with pytest.raises(ValueError):
        ctx.shade_rays_device(rays, samples=0)
    # n_points == 0: nothing is enqueued, nothing written
    sentinel = torch.full((64, 4), 7.25, device="cuda:0")
    assert _call(ctx, 0, 1, None, sentinel, sentinel) == 0
    assert _call(ctx, 0, 3, rays, sentinel, None) == 0
    s, p = ctx.shade_rays_device(torch.zeros((0, 8), dtype=torch.float32, device="cuda:0"))
    torch.cuda.synchronize()
    assert s.shape == (0, 4) and p.shape == (0, 4)
    assert (sentinel == 7.25).all()
    # trace_variant != 0 (the alt library has the other variants)
    alt = RtContext(0, variant="alt")
    try:
        alt.set_param("trace_variant", 2)
        assert _call(alt, 16, 1, rays, so, po) == E
    finally:
        alt.close()


@pytest.mark.gpu
def test_not_ready(ctx):
    import torch
    from tests.test_blas_refit import deform
    rays = dev(scenes.random_rays(64, seed=3))
    so = torch.empty((64, 4), dtype=torch.float32, device="cuda:0")
    NR = RT_ERR_NOT_READY
    c = RtContext(0)
    try:
        assert _call(c, 64, 1, rays, so, None) == NR                   # no uniforms, no geometry
        sp = mixed_scene(2, 1)
        c.set_uniforms(sp.uniforms)
        assert _call(c, 64, 1, rays, so, None) == NR                   # no geometry
        c.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        assert _call(c, 64, 1, rays, so, None) == NR                   # no TLAS
        c.set_instances(sp.instances)
        assert _call(c, 64, 1, rays, so, None) == 0
        torch.cuda.synchronize()
        t = deform(sp.geom, 0, amp=0.1)
        torch.cuda.synchronize()
        c.refit_blas_device(0, t)
        assert _call(c, 64, 1, rays, so, None) == NR                   # TLAS stale after a refit
        c.set_instances(sp.instances, update=True)
        assert _call(c, 64, 1, rays, so, None) == 0
        torch.cuda.synchronize()
        c.set_batch(np.stack([sp.instances, sp.instances]), np.concatenate([sp.uniforms, sp.uniforms]))
        assert _call(c, 64, 1, rays, so, None) == NR                   # a frame batch held
        c.set_instances(sp.instances)
        assert _call(c, 64, 1, rays, so, None) == 0
        torch.cuda.synchronize()
    finally:
        c.close()


# ---- 8. ordering --------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rays_written_on_a_side_stream(ctx):
    import torch
    sp = mixed_scene(4, 1, ctx=ctx)
    host_rays = arbitrary_rays(sp, seed=9)
    ref_s, ref_p = shade(ctx, host_rays, samples=1)
    src = dev(host_rays)
    side = torch.cuda.Stream()
    rays = torch.empty_like(src)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(200_000_000)
        rays.copy_(src)
        s, p = ctx.shade_rays_device(rays, stream=side)
    assert not side.query()   # the call returned before the rays were written
    side.synchronize()
    assert same(s.cpu().numpy(), ref_s) and same(p.cpu().numpy(), ref_p)
    assert same(ref_s, shade_samples(sp.orc, host_rays, len(host_rays), 4))
    # the TLAS of the call, whatever rt_set_instances does right after it
    other = sp.instances.copy()
    for k in range(len(other)):
        other[k]["transform"][3] += 2.5
    with torch.cuda.stream(side):
        torch.cuda._sleep(200_000_000)
        s, p = ctx.shade_rays_device(src, stream=side)
    ctx.set_instances(other)
    ctx.set_instances(other, update=True)
    side.synchronize()
    assert same(s.cpu().numpy(), ref_s) and same(p.cpu().numpy(), ref_p)
    s2, _ = shade(ctx, src)
    assert not same(s2, ref_s)   # (the new instances do change the colours)
    ctx.set_instances(sp.instances)


@pytest.mark.gpu
def test_beside_a_pending_frame(ctx):
    sp = mixed_scene(4, 2, ctx=ctx)
    W, H = 160, 90
    frame, _ = ctx.trace(W, H)
    rays = arbitrary_rays(sp, seed=11)
    ref_s, ref_p = shade(ctx, rays)
    import torch
    t = dev(rays)
    ctx.trace_async(W, H)
    s, p = ctx.shade_rays_device(t)
    img, _ = ctx.trace_wait()
    torch.cuda.synchronize()
    assert same(img, frame)
    assert same(s.cpu().numpy(), ref_s) and same(p.cpu().numpy(), ref_p)


@pytest.mark.gpu
def test_two_streams_growth_and_queries():
    """two calls back to back on two streams, the second larger than the first (the queues grow), with device ray queries
    between them: each result equals its standalone result"""
    import torch
    c = RtContext(0)
    try:
        sp = mixed_scene(5, 1, ctx=c)
        small = arbitrary_rays(sp, seed=21)[:900]
        big = np.concatenate([arbitrary_rays(sp, seed=22)] * 6)
        qrays = scenes.random_rays(5000, seed=23)
        ref_small = shade_samples(sp.orc, small, len(small), 5)
        ref_big = shade_samples(sp.orc, big[:len(big) // 3 * 3], len(big) // 3, 5)
        qref, _ = c.intersect(qrays)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        ts, tb, tq = dev(small), dev(big[:len(big) // 3 * 3]), dev(qrays)
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            torch.cuda._sleep(100_000_000)
            q1 = c.intersect_device(tq, stream=s1)
            a = c.shade_rays_device(ts, stream=s1)
        with torch.cuda.stream(s2):
            b = c.shade_rays_device(tb, samples=3, stream=s2)
            q2 = c.intersect_device(tq, stream=s2)
        with torch.cuda.stream(s1):
            a2 = c.shade_rays_device(ts, stream=s1, points=False)
        torch.cuda.synchronize()
        assert same(a[0].cpu().numpy(), ref_small) and same(a2[0].cpu().numpy(), ref_small)
        assert same(b[0].cpu().numpy(), ref_big)
        assert same(b[1].cpu().numpy(), average_points(ref_big, len(big) // 3, 3))
        for q in (q1, q2):
            assert q.numpy()[0].tobytes() == qref.tobytes()
    finally:
        c.close()
