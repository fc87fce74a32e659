"""rt_set_instances_device: the TLAS built (LBVH) and refitted on the GPU from instance records in device memory.

The closest hit does not depend on the tree, so every frame and every closest-hit record through the device
path must be bit-identical to the host path's (rt_set_instances, binned SAH on the host) fed the same bytes."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import scenes
from tests.exact import assert_frame_equals_oracle
from vulkan_raytracing_amd import RtContext, api, host, workloads
from vulkan_raytracing_amd.api import INSTANCE_DTYPE, RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = scenes.RES
PATHS = [os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj")]
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_product_library_exports_set_instances_device():
    assert "rt_set_instances_device" in api.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^int rt_set_instances_device\(rt_ctx\* ctx, const void\* d_instances, int n, int update, void\* hip_stream\);", hdr, re.M)
    L = api.lib()
    assert hasattr(L, "rt_set_instances_device")
    assert L.rt_abi_version() == 7


def test_null_context_is_rejected_without_a_device():
    L = api.lib()
    assert L.rt_set_instances_device(None, None, 1, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_set_instances_device(None, None, 0, 1, None) == RT_ERR_INVALID_ARGUMENT


def test_per_frame_tlas_kernels_use_no_scratch():
    """`make resource-usage-tlas` (hipcc -Rpass-analysis=kernel-resource-usage over tlas_gpu.hip, a cross-compile): the kernels every
    device TLAS build or refit launches keep everything in registers."""
    out = subprocess.run(["make", "-C", ROOT, "resource-usage-tlas"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    for short in ("k_inst_records", "k_tlas_refit", "k_tlas_emit", "k_tlas_far", "k_tlas_quant", "k_morton", "k_radix_tree"):
        found = [(n, r) for n, r in kernels.items() if short in n]
        assert found, (short, list(kernels))
        for name, r in found:
            assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

def _dev(inst):
    import torch
    b = np.ascontiguousarray(inst, INSTANCE_DTYPE).view(np.uint8).reshape(-1, 64)
    return torch.from_numpy(b.copy()).to("cuda:0")


def _set_dev(ctx, inst, update=False):
    import torch
    t = _dev(inst)
    torch.cuda.current_stream().synchronize()
    ctx.set_instances_device(t, update=update)


def _rot(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def instance_field(n, seed, extent=14.0, scale=(0.05, 0.35)):
    """n seeded instances of mesh 0 (teapot) and 1 (cube): random positions, rotations, non-uniform scales, shears, mirrored
    transforms (negative determinant) and some mask-0 instances"""
    rng = np.random.default_rng(seed)
    inst = np.zeros(n, INSTANCE_DTYPE)
    for i in range(n):
        M = _rot(rng) @ np.diag(rng.uniform(*scale, 3))
        if i % 5 == 1:
            M = M @ np.array([[1, rng.uniform(-0.6, 0.6), 0], [0, 1, rng.uniform(-0.6, 0.6)], [0, 0, 1]])
        if i % 7 == 2:
            M = M @ np.diag([-1.0, 1.0, 1.0])
        t = rng.uniform(-extent, extent, 3)
        mesh = int(rng.integers(0, 2))
        inst[i] = host.make_instance(np.concatenate([M, t[:, None]], axis=1).astype(np.float32).reshape(12), mesh, mesh)
        if i % 17 == 3:
            inst[i]["custom_index_and_mask"] = inst[i]["custom_index_and_mask"] & 0xFFFFFF   # mask 0: never hit
    return inst


def field_uniforms(geom, max_bounce=2, spp=1):
    return host.default_uniforms(max_bounce_count=max_bounce, samples_per_pixel=spp, center_object_type=1, orbiting_object_type=0,
                                 orbiting_object_primitive_offset=geom.orbiting_primitive_offset, orbiting_object_vertex_offset=geom.orbiting_vertex_offset)


@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_cfg5_ring_device_equals_host_and_oracle(ctx):
    w = workloads.make("cfg5", RES)
    sp = scenes.ScenePair(w.paths, w.instances, w.uniforms, sky=w.sky, ctx=ctx)
    W, H = 240, 136
    host_img, st_h = ctx.trace(W, H)
    _set_dev(ctx, w.instances)
    dev_img, st_d = ctx.trace(W, H)
    assert np.array_equal(dev_img.view(np.uint32), host_img.view(np.uint32))
    assert (st_d.rays_primary, st_d.rays_secondary, st_d.rays_shadow) == (st_h.rays_primary, st_h.rays_secondary, st_h.rays_shadow)
    ref, rc = sp.orc.render(W, H)
    assert_frame_equals_oracle(dev_img, sp.orc, W, H, ref=ref)
    assert (st_d.rays_primary, st_d.rays_secondary, st_d.rays_shadow) == tuple(int(x) for x in rc)


@pytest.mark.gpu
def test_instance_field_hit_records_and_frame(ctx):
    inst = instance_field(4096, seed=3)
    geom = host.SceneGeometry(PATHS)
    sp = scenes.ScenePair(PATHS, inst, field_uniforms(geom), sky=scenes.synthetic_skybox(64), ctx=ctx)
    rays = scenes.random_rays(100_000, seed=9, origin_radius=40.0, target_radius=14.0)
    shadow = rays.copy(); shadow[:, 7] = 30.0
    g_host, _ = ctx.intersect(rays)
    a_host, _ = ctx.intersect(shadow, any_hit=True)
    W, H = 320, 180
    img_host, _ = ctx.trace(W, H)
    _set_dev(ctx, inst)
    g_dev, _ = ctx.intersect(rays)
    a_dev, _ = ctx.intersect(shadow, any_hit=True)
    img_dev, _ = ctx.trace(W, H)
    assert (g_host["inst"] >= 0).mean() > 0.2 and not np.any(np.isin(g_dev["inst"], np.arange(3, 4096, 17)))
    assert g_dev.tobytes() == g_host.tobytes()
    # any hit: whether the segment is blocked (which of several blockers a walk meets first depends on the tree)
    assert np.array_equal(a_dev["inst"] >= 0, a_host["inst"] >= 0)
    assert np.array_equal(img_dev.view(np.uint32), img_host.view(np.uint32))
    sub = np.random.default_rng(4).choice(len(rays), 48, replace=False)
    o = sp.orc.intersect(rays[sub], use_bvh=False)
    assert o.tobytes() == g_dev[sub].tobytes()


def grid_field(n, spacing=0.5):
    """n small cubes and teapots on a cubic lattice (no overlaps): a field of many instances at a cheap frame"""
    side = int(np.ceil(n ** (1 / 3)))
    i = np.arange(n)
    pos = (np.stack([i % side, (i // side) % side, i // (side * side)], axis=1) - (side - 1) / 2.0) * spacing
    inst = np.zeros(n, INSTANCE_DTYPE)
    base = [host.make_instance(np.array([0.08, 0, 0, 0, 0, 0.08, 0, 0, 0, 0, 0.08, 0], np.float32), m, m) for m in (0, 1)]
    for m in (0, 1):
        sel = (i % 2) == m
        inst[sel] = base[m]
    tr = inst["transform"]
    tr[:, 3], tr[:, 7], tr[:, 11] = pos[:, 0], pos[:, 1], pos[:, 2]
    inst["transform"] = tr
    return inst


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65535, 262144])
def test_large_instance_counts(ctx, n, capfd, monkeypatch):
    inst = grid_field(n)
    geom = host.SceneGeometry(PATHS)
    scenes.ScenePair(PATHS, inst[:1], field_uniforms(geom, max_bounce=1), sky=scenes.synthetic_skybox(64), ctx=ctx)
    W, H = 160, 96
    ctx.set_instances(inst)
    img_host, _ = ctx.trace(W, H)
    monkeypatch.setenv("RT_BUILD_TIMING", "1")
    _set_dev(ctx, inst)
    err = capfd.readouterr().err
    m = re.search(r"\[tlas_gpu\] %d instances, LBVH build, depth (\d+)" % n, err)
    assert m, err
    print("device LBVH over %d instances: depth %s" % (n, m.group(1)))
    img_dev, _ = ctx.trace(W, H)
    assert (img_host != img_host[0, 0]).any()
    assert np.array_equal(img_dev.view(np.uint32), img_host.view(np.uint32))


@pytest.mark.gpu
def test_refit_frames_equal_host_and_rebuild(ctx):
    n = 512
    inst0 = instance_field(n, seed=8, extent=10.0, scale=(0.2, 0.8))
    geom = host.SceneGeometry(PATHS)
    u = field_uniforms(geom)
    hctx = RtContext(0)
    try:
        scenes.ScenePair(PATHS, inst0, u, sky=scenes.synthetic_skybox(64), ctx=hctx)
        scenes.ScenePair(PATHS, inst0, u, sky=scenes.synthetic_skybox(64), ctx=ctx)
        _set_dev(ctx, inst0)
        rng = np.random.default_rng(1)
        vel = rng.normal(size=(n, 3)).astype(np.float32)
        W, H = 200, 112
        for k in range(8):
            inst = inst0.copy()
            tr = inst["transform"]
            for a, col in enumerate((3, 7, 11)):
                tr[:, col] += np.float32(0.4 * (k + 1)) * vel[:, a]
            inst["transform"] = tr
            hctx.set_instances(inst, update=True)
            img_h, _ = hctx.trace(W, H)
            _set_dev(ctx, inst, update=True)
            img_refit, _ = ctx.trace(W, H)
            assert np.array_equal(img_refit.view(np.uint32), img_h.view(np.uint32)), k
            if k % 3 == 2:
                _set_dev(ctx, inst, update=False)       # a device rebuild gives the same frame; refits continue from it
                img_rb, _ = ctx.trace(W, H)
                assert np.array_equal(img_rb.view(np.uint32), img_h.view(np.uint32)), k
        with pytest.raises(RtError) as e:
            _set_dev(ctx, inst0[:n - 1], update=True)   # a different n
        assert e.value.code == RT_ERR_INVALID_ARGUMENT
        ctx.set_instances(inst0)
        with pytest.raises(RtError) as e:
            _set_dev(ctx, inst0, update=True)           # after a host build
        assert e.value.code == RT_ERR_INVALID_ARGUMENT
        _set_dev(ctx, inst0)
        with pytest.raises(RtError) as e:
            ctx.set_instances(inst0, update=True)       # a host refit of a device build
        assert e.value.code == RT_ERR_INVALID_ARGUMENT
    finally:
        hctx.close()


@pytest.mark.gpu
def test_stream_order_and_ownership(ctx):
    import torch
    inst = instance_field(1024, seed=12)
    geom = host.SceneGeometry(PATHS)
    scenes.ScenePair(PATHS, inst, field_uniforms(geom), sky=scenes.synthetic_skybox(64), ctx=ctx)
    W, H = 200, 112
    img_host, _ = ctx.trace(W, H)
    words = torch.from_numpy(inst.view(np.int32).reshape(-1, 16).copy()).to("cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        # a queue of work in front of the records, then the records themselves produced by torch ops on that stream
        a = torch.randn(2048, 2048, device="cuda:0")
        for _ in range(8):
            a = a @ a / 64.0
        rec = (words + (a[0, 0] != a[0, 0]).to(torch.int32) * 0).contiguous()
        ctx.set_instances_device(rec.view(torch.uint8), stream=s)   # no synchronisation by the caller
        rec.zero_()                                                 # overwritten right after the call, on the same stream
    img_dev, _ = ctx.trace(W, H)
    torch.cuda.synchronize()
    assert np.array_equal(img_dev.view(np.uint32), img_host.view(np.uint32))


@pytest.mark.gpu
def test_pending_frame_keeps_its_instances(ctx):
    geom = host.SceneGeometry(PATHS)
    a = instance_field(256, seed=21)
    b = instance_field(256, seed=22)
    scenes.ScenePair(PATHS, a, field_uniforms(geom), sky=scenes.synthetic_skybox(64), ctx=ctx)
    W, H = 200, 112
    img_a, _ = ctx.trace(W, H)
    ctx.set_instances(b)
    img_b, _ = ctx.trace(W, H)
    assert not np.array_equal(img_a, img_b)
    _set_dev(ctx, a)
    for _ in range(2):
        ctx.trace_async(W, H)
        _set_dev(ctx, b)                   # the frame in flight still reads the records it was submitted with
        pending, _ = ctx.trace_wait()
        assert np.array_equal(pending.view(np.uint32), img_a.view(np.uint32))
        nxt, _ = ctx.trace(W, H)
        assert np.array_equal(nxt.view(np.uint32), img_b.view(np.uint32))
        _set_dev(ctx, a)


@pytest.mark.gpu
def test_instance_types_reissue_and_builder_switch(ctx):
    geom = host.SceneGeometry(PATHS)
    inst = instance_field(300, seed=31, scale=(0.3, 0.9))
    scenes.ScenePair(PATHS, inst, field_uniforms(geom, max_bounce=3), sky=scenes.synthetic_skybox(64), ctx=ctx)
    W, H = 200, 112
    try:
        for types in (np.arange(300) % 3, (np.arange(300) // 7) % 3):
            ctx.set_instances(inst)
            ctx.set_instance_types(types.astype(np.uint32))
            img_h, _ = ctx.trace(W, H)
            _set_dev(ctx, inst)
            img_d, _ = ctx.trace(W, H)
            assert np.array_equal(img_d.view(np.uint32), img_h.view(np.uint32))
        _set_dev(ctx, inst)
        ctx.set_instance_types((np.arange(300) % 3).astype(np.uint32))   # re-issued from the library's copy of the records
        img_d, _ = ctx.trace(W, H)
        ctx.set_instances(inst)
        img_h, _ = ctx.trace(W, H)
        assert np.array_equal(img_d.view(np.uint32), img_h.view(np.uint32))
        _set_dev(ctx, inst)
        ctx.set_param("blas_builder", 0)
        img_d2, _ = ctx.trace(W, H)
        assert np.array_equal(img_d2.view(np.uint32), img_h.view(np.uint32))
    finally:
        ctx.set_param("blas_builder", 1)
        ctx.set_instance_types(None)


@pytest.mark.gpu
def test_far_camera(ctx):
    geom = host.SceneGeometry(PATHS)
    inst = instance_field(256, seed=41, scale=(2.0, 6.0), extent=200.0)
    u = field_uniforms(geom)
    u["position"][0][:3] = (0.0, 0.0, 5000.0)
    scenes.ScenePair(PATHS, inst, u, sky=scenes.synthetic_skybox(64), ctx=ctx)
    W, H = 200, 112
    img_h, _ = ctx.trace(W, H)
    _set_dev(ctx, inst)
    img_d, _ = ctx.trace(W, H)
    assert np.array_equal(img_d.view(np.uint32), img_h.view(np.uint32))


@pytest.mark.gpu
def test_errors(ctx):
    import torch
    geom = host.SceneGeometry(PATHS)
    inst = instance_field(64, seed=51)
    sp = scenes.ScenePair(PATHS, inst, field_uniforms(geom), sky=scenes.synthetic_skybox(64), ctx=ctx)
    W, H = 64, 48
    bad = inst.copy(); bad[10]["mesh"] = 7
    with pytest.raises(RtError) as e:
        _set_dev(ctx, bad)
    assert e.value.code == RT_ERR_INVALID_ARGUMENT and "unknown mesh" in str(e.value)
    with pytest.raises(RtError) as e:
        ctx.trace(W, H)
    assert e.value.code == RT_ERR_NOT_READY
    t = _dev(inst)
    torch.cuda.synchronize()
    assert ctx.L.rt_set_instances_device(ctx.h, None, 64, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert ctx.L.rt_set_instances_device(ctx.h, t.data_ptr(), 0, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert ctx.L.rt_set_instances_device(ctx.h, t.data_ptr(), -3, 0, None) == RT_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        ctx.set_instances_device(t[:, :32].contiguous())
    with pytest.raises(ValueError):
        ctx.set_instances_device(t.cpu())
    # an instance of a mesh whose BLAS is not built
    ctx.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges, build=False)
    ctx.build_blas(0)
    with pytest.raises(RtError) as e:
        ctx.set_instances_device(t)
    assert e.value.code == RT_ERR_NOT_READY
    with pytest.raises(RtError) as e:
        ctx.trace(W, H)
    assert e.value.code == RT_ERR_NOT_READY
    ctx.build_blas(1)
    ctx.set_instances_device(t)
    img, _ = ctx.trace(W, H)
    ctx.set_instances(inst)
    img_h, _ = ctx.trace(W, H)
    assert np.array_equal(img.view(np.uint32), img_h.view(np.uint32))
