"""rt_set_param's launch tunables are result-identical (include/rt_api.h: "Results do not depend on any of them").

They size the persistent grids, the device-side trimming of k_trace's grid, the per-launch caps of the closest-hit and shadow
launches and the entry records; the grids in turn size the spill areas of the frame and of the query workspace, which the kernels
index per thread of the launched grid.  Under every setting a frame must equal the oracle bit for bit (tests/exact.py) and the
frame of a context left at the defaults, with the same ray counts; under the smallest and the largest grids the ray queries, the
shading of caller-generated rays and a frame batch must equal the default context's results too.  trace_blocks_per_cu cannot be
set back to its automatic value, so every setting gets a context of its own."""
import os

import numpy as np
import pytest

from tests import scenes, stack_reference
from tests.exact import assert_frame_equals_oracle, assert_hits_equal_oracle
from tests.shade_reference import pinhole_rays
from vulkan_raytracing_amd import RtContext, api, host, tiling
from vulkan_raytracing_amd.api import INSTANCE_DTYPE, RtError

pytestmark = pytest.mark.gpu
RES = scenes.RES
W, H = 263, 151                 # not multiples of the 8x8 tile
RT_ERR_INVALID_ARGUMENT = 1
MINIMAL = {"trace_blocks_per_cu": 1, "trace_rays_per_lane": 64, "shade_blocks_per_cu": 1}
MAXIMAL = {"trace_blocks_per_cu": 8, "trace_rays_per_lane": 1, "shade_blocks_per_cu": 16, "trace_min_blocks": 4096}
BAND, SHARD, N_SHARDS, K = 8, 1, 3, 3
TYPES = [1] + [2 if k % 3 == 0 else 0 for k in range(16)]    # the mirror cube, glass and diffuse teapots


def make_scene(ctx=None):
    """cfg5's ring (16 teapots about a mirror cube: 17 instances), every third teapot glass, depth 4, spp 3, a sky"""
    sp = scenes.ring_scene(os.path.join(RES, "teapot.obj"), 16, 10.0, 4, 3, sky=scenes.synthetic_skybox(64), ctx=ctx,
                           center_path=os.path.join(RES, "cube.obj"))
    sp.set_instance_types(TYPES)
    return sp


def counts(st):
    return (st.rays_primary, st.rays_secondary, st.rays_shadow)


def query_inputs():
    rays = scenes.random_rays(6000, seed=71, target_radius=12.0)
    sh = rays.copy(); sh[:, 7] = 25.0
    words = np.random.default_rng(72).integers(0, 1 << 32, len(rays), dtype=np.uint64).astype(np.uint32)
    words &= np.uint32(0xFF0003FF)                     # bits 0-9 ray flags, 24-31 cull mask
    words[::5] = 0xFF000000                            # plain rays in between
    return rays, sh, words


def run_queries(ctx, rays, sh, words):
    import torch
    d = torch.from_numpy(rays).to("cuda:0")
    ds = torch.from_numpy(sh).to("cuda:0")
    dw = torch.from_numpy(words.view(np.int32)).to("cuda:0")
    closest = ctx.intersect_device(d, attributes=True)
    first = ctx.intersect_device(ds, any_hit=True)
    flags = ctx.intersect_device_flags(d, words=dw, attributes=True)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (closest.hits, closest.attr, first.hits, flags.hits, flags.attr)]


def run_shade(ctx, rays):
    import torch
    s, p = ctx.shade_rays_device(torch.from_numpy(rays).to("cuda:0"), samples=3)
    torch.cuda.synchronize()
    return s.cpu().numpy(), p.cpu().numpy()


def batch_inputs(sp):
    """K frames of the scene with their own camera and light"""
    us = []
    for k in range(K):
        u = sp.uniforms.copy()
        u[0]["position"][:3] = (0.4 * k - 0.5, 0.3 * k, 20.0 - 0.7 * k)
        u[0]["light_position"][:3] = (5.0 - k, 5.0 + 0.5 * k, 5.0)
        us.append(u)
    return np.stack([sp.instances] * K), np.concatenate(us)


def run_batch(ctx, sp, binst, bu):
    import torch
    rows = tiling.max_shard_rows(H, BAND, N_SHARDS)
    ctx.set_batch(binst, bu)
    buf = torch.zeros((K, rows, W, 4), dtype=torch.float32, device="cuda:0")
    ctx.trace_shard_batch(W, H, BAND, SHARD, N_SHARDS, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream,
                          frame_stride_bytes=rows * W * 16)
    st = ctx.stats()
    out = buf.cpu().numpy()
    ctx.set_instances(sp.instances)                    # back to single frames
    ctx.set_uniforms(sp.uniforms)
    return out, counts(st)


@pytest.fixture(scope="module")
def base():
    """the default context's results, and the oracle's frame"""
    c = RtContext(0)
    try:
        sp = make_scene(c)
        img, st = c.trace(W, H)
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(img, sp.orc, W, H, ref=ref)
        assert counts(st) == tuple(int(x) for x in rc) and st.rays_secondary > 0 and st.rays_shadow > 0
        q_in = query_inputs()
        prays = pinhole_rays(sp.orc, W, H, 3)
        binst, bu = batch_inputs(sp)
        yield dict(sp=sp, img=img, ref=ref, counts=counts(st), q_in=q_in, q=run_queries(c, *q_in), prays=prays,
                   shade=run_shade(c, prays), binst=binst, bu=bu, batch=run_batch(c, sp, binst, bu))
    finally:
        c.close()


def fresh(params):
    c = RtContext(0)
    try:
        for k, v in params.items():
            c.set_param(k, v)
    except BaseException:
        c.close()
        raise
    return c


def check_frame(c, base):
    img, st = c.trace(W, H)
    assert_frame_equals_oracle(img, base["sp"].orc, W, H, ref=base["ref"])
    assert np.array_equal(img.view(np.uint32), base["img"].view(np.uint32))
    assert counts(st) == base["counts"]
    return img


@pytest.mark.parametrize("grid", ["minimal", "maximal"])
def test_persistent_grid_sizes(base, grid):
    c = fresh(MINIMAL if grid == "minimal" else MAXIMAL)
    try:
        make_scene(c)
        check_frame(c, base)
        q = run_queries(c, *base["q_in"])
        for a, b in zip(q, base["q"]):
            assert np.array_equal(a, b), grid
        assert_hits_equal_oracle(q[0].view(api.HIT_DTYPE).reshape(-1), base["sp"].orc, base["q_in"][0])
        s, p = run_shade(c, base["prays"])
        assert np.array_equal(s.view(np.uint32), base["shade"][0].view(np.uint32))
        assert np.array_equal(p.view(np.uint32), base["shade"][1].view(np.uint32))
        assert np.array_equal(p.reshape(H, W, 4).view(np.uint32), base["img"].view(np.uint32))   # the frame's own shading
        out, rays = run_batch(c, base["sp"], base["binst"], base["bu"])
        assert np.array_equal(out.view(np.uint32), base["batch"][0].view(np.uint32)) and rays == base["batch"][1]
        check_frame(c, base)                           # and single frames again after the batch
    finally:
        c.close()


@pytest.mark.parametrize("name", ["closest_blocks_per_cu", "shadow_blocks_per_cu"])
@pytest.mark.parametrize("value", [0, 1, 8])
def test_launch_caps_on_the_root_of_four_frame_slots(base, name, value):
    root = RtContext(0)
    slots = []
    try:
        sp = make_scene(root)
        slots = [root.frame_slot() for _ in range(3)]
        for s in slots:
            s.set_instance_types(TYPES)
            s.set_instances(sp.instances)
            s.set_uniforms(sp.uniforms)
        root.set_param(name, value)
        for s in slots:
            s.trace_async(W, H)                        # three frames pending while the root renders
        check_frame(root, base)
        for s in slots:
            img, st = s.trace_wait()
            assert np.array_equal(img.view(np.uint32), base["img"].view(np.uint32)) and counts(st) == base["counts"]
    finally:
        for s in reversed(slots):
            s.close()
        root.close()


@pytest.mark.parametrize("params", [{"camera_records": 0}, {"entry_max_instances": 1}, {"entry_max_instances": 64}],
                         ids=["camera_records_0", "entry_max_instances_1", "entry_max_instances_64"])
def test_entry_record_settings(base, params):
    c = fresh(params)
    try:
        make_scene(c)
        assert len(base["sp"].instances) >= 17
        check_frame(c, base)
    finally:
        c.close()


@pytest.mark.parametrize("tiles", [8, 512])
def test_light_tiles_with_kept_shadow_records(base, tiles):
    c = fresh({"light_tiles": tiles, "shadow_entry": 2})
    try:
        make_scene(c)
        for _ in range(3):                             # built once the light and the instances stood still, then kept and used
            check_frame(c, base)
    finally:
        c.close()


def deep_mesh(path, n=96, s=0.5):
    """triangles facing +z about the z axis, each half the size of the one before and nearer the origin: the host builder's tree
    peels them off one or two at a time, and rays close to the axis walk all of it"""
    with open(path, "w") as f:
        for k in range(n):
            a = 4.0 * s ** k
            for v in ((-a, -a, -a), (3.0 * a, -a, -a), (-a, 3.0 * a, -a)):
                f.write("v %.9g %.9g %.9g\nvn 0 0 1\n" % v)
        for k in range(n):
            f.write("f %d//%d %d//%d %d//%d\n" % (3 * k + 1, 3 * k + 1, 3 * k + 2, 3 * k + 2, 3 * k + 3, 3 * k + 3))


def axis_rays(n, seed):
    """rays down the z axis that pass within 1e-17 .. 1e-15 of it: they enter the boxes of triangles down to that size"""
    rng = np.random.default_rng(seed)
    r = 10.0 ** rng.uniform(-17, -15, n)
    phi = rng.uniform(0, 2 * np.pi, n)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0] = r * np.cos(phi); rays[:, 1] = r * np.sin(phi); rays[:, 2] = 20.0
    rays[:, 3] = 0.001
    rays[:, 4] = rng.uniform(-1e-20, 1e-20, n); rays[:, 5] = rng.uniform(-1e-20, 1e-20, n); rays[:, 6] = -1.0
    rays[:, 7] = 10000.0
    return rays


CORRIDOR = 8192                 # squares of the frame's corridor: 12 levels, 14 stack entries with the sentinel and the marker (the oracle visits half the tree per ray)


DEEP_W, DEEP_H = 1024, 640      # more pixels than the threads of the resident part of the largest grid


def test_spill_areas_grow_with_the_grid(tmp_path):
    """Two host-built trees: a 40-level one (deep_mesh: its spill area per thread is wider than the smallest) that the queries walk
    along its axis, and a corridor (scenes.corridor: a row of squares whose tree a ray along the row walks with one stack entry per
    level) that fills the frame, so that every primary ray of the frame spills (its walk starts at the TLAS root: camera_records 0);
    the model of tests/stack_reference.py says so for a sample of them, on this context's own trees.  A frame and a query on the
    smallest grid (trace_blocks_per_cu 1), then on the largest, with
    trace_rays_per_lane 1 and trace_min_blocks above the grid so that k_trace trims none of it.  The work is handed out in chunks (64
    rays, or a run of pixels) to every wave that starts, and there are more rays than the resident part of the grid has threads (524288 query rays,
    655360 pixels), so workgroups beyond the first grid's walk deep rays too: both spill areas, the frame's and the query
    workspace's, must have grown with the grid."""
    import torch
    deep, chain = str(tmp_path / "deep.obj"), str(tmp_path / "corridor.obj")
    deep_mesh(deep)
    cv, ci = scenes.corridor(CORRIDOR, spacing=0.0005)  # 4.1 long: the rays of the frame's corners stay inside its footprint to the end
    cv[:, 0] += 110.0; cv[:, 1] += 10.0                 # x 102 .. 118, y 2 .. 18: out of the deep mesh's way
    scenes.write_obj(chain, cv, ci)
    for path, depth in ((deep, 40), (chain, 12)):
        g = host.SceneGeometry([path])
        rc, info = api.check_builders(g.verts, g.idx)
        assert rc == 0 and info["depth"] >= depth, (path, info)
    c = RtContext(0)
    try:
        c.set_param("blas_builder", 0)
        c.set_param("trace_blocks_per_cu", 1)
        c.set_param("camera_records", 0)
        ident = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
        inst = [host.make_instance(ident, 0, 0), host.make_instance(ident, 1, 1)]
        geom = host.SceneGeometry([deep, chain])
        u = host.default_uniforms(max_bounce_count=1, samples_per_pixel=1, center_object_type=0, orbiting_object_type=0,
                                  orbiting_object_primitive_offset=geom.orbiting_primitive_offset,
                                  orbiting_object_vertex_offset=geom.orbiting_vertex_offset)
        u[0]["position"][:3] = (110.0, 10.0, 2.5)          # looking down the corridor, which fills the view; the deep mesh lies out of it
        u[0]["light_position"][:3] = (110.0, 13.0, 10.0)
        sp = scenes.ScenePair([deep, chain], np.asarray(inst, INSTANCE_DTYPE), u, sky=scenes.synthetic_skybox(32), ctx=c)
        rays = axis_rays(1 << 19, seed=5)
        bf = sp.orc.intersect(rays, use_bvh=False)
        assert (bf["inst"] == 0).all()    # (the nearest triangles' distances round to the same t: the tie rule picks among them)
        ref, rc = sp.orc.render(DEEP_W, DEEP_H)
        assert rc[0] == DEEP_W * DEEP_H and rc[2] > DEEP_W * DEEP_H // 2
        xy = [(x, y) for x in (0, DEEP_W // 2, DEEP_W - 1) for y in (0, DEEP_H // 2, DEEP_H - 1)]   # the corners and the centre
        prim = np.zeros((len(xy), 8), np.float32)
        for i, (x, y) in enumerate(xy):
            od = sp.orc.primary_ray(x, y, DEEP_W, DEEP_H, 0)
            prim[i] = (od[0], od[1], od[2], 0.001, od[3], od[4], od[5], 10000.0)
        assert (sp.orc.intersect(prim, use_bvh=False)["inst"] == 1).all()    # the corridor fills the frame
        model = stack_reference.StackModel(c.debug_snapshot())
        peaks = [model.first(q) for q in stack_reference.rays_of(prim)]
        assert stack_reference.stack2_lds() == 12 and min(peaks) >= 12 + 2, peaks       # every one of them spills
        for params in ({}, {"trace_blocks_per_cu": 8, "trace_rays_per_lane": 1, "trace_min_blocks": 4096}):
            for k, v in params.items():
                c.set_param(k, v)
            img, st = c.trace(DEEP_W, DEEP_H)
            assert_frame_equals_oracle(img, sp.orc, DEEP_W, DEEP_H, ref=ref)
            assert counts(st) == tuple(int(x) for x in rc)
            h, _ = c.intersect_device(torch.from_numpy(rays).to("cuda:0")).numpy()
            assert np.array_equal(h.view(np.uint8), bf.view(np.uint8)), params
    finally:
        c.close()


REFUSED = [("trace_blocks_per_cu", 0), ("trace_blocks_per_cu", 9), ("trace_rays_per_lane", 0), ("trace_rays_per_lane", 65),
           ("trace_min_blocks", 7), ("shade_blocks_per_cu", 0), ("shade_blocks_per_cu", 17), ("closest_blocks_per_cu", -2),
           ("closest_blocks_per_cu", 9), ("shadow_blocks_per_cu", -2), ("shadow_blocks_per_cu", 9), ("entry_max_instances", 0),
           ("light_tiles", 7), ("light_tiles", 513), ("shadow_entry", 3), ("shadow_entry", -1)]


def test_out_of_range_values_are_refused_and_change_nothing(base):
    """each refused call returns RT_ERR_INVALID_ARGUMENT, and a context that refused them all still renders the default frame with
    the same ray counts and answers the queries as before (on a context whose grid was set to the smallest one first).  Results do
    not depend on the tunables, so this shows that a refused call breaks nothing, not which value is in force."""
    c = fresh(MINIMAL)
    try:
        make_scene(c)
        c.set_param("light_tiles", 64)
        c.set_param("entry_max_instances", 20)
        for name, value in REFUSED:
            with pytest.raises(RtError) as e:
                c.set_param(name, value)
            assert e.value.code == RT_ERR_INVALID_ARGUMENT, (name, value)
        with pytest.raises(RtError) as e:
            c.set_param("entry_max_instances", 1 << 30)
        assert e.value.code == RT_ERR_INVALID_ARGUMENT
        check_frame(c, base)
        q = run_queries(c, *base["q_in"])
        for a, b in zip(q, base["q"]):
            assert np.array_equal(a, b)
    finally:
        c.close()
