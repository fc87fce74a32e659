"""Sky tiles, the all-miss marker and the per-run origin of the pixel runs (k_raygen / k_beam / k_resolve), frame against oracle.

A tile of 8x8 pixels that no mesh can touch (coverage mask, empty entry record) is finished by k_raygen, which stores its pixels and
nothing else, and skipped by k_resolve — both ask the same predicate; an all-miss pixel inside a covered tile still takes the PIXEL_DONE marker; with pixel runs
(the default) queue 0 holds one origin per run instead of one per ray.  Every frame below is compared with the oracle's BIT FOR BIT
(tests/exact.py, no tolerance), on frames small enough for the oracle and shaped so that every path is taken:

  scene    one cube (half size 1), off-centre, the camera 9 in front of the origin: about 24 pixels across in a 70-pixel frame, so a
           frame has sky tiles, covered tiles with all-miss pixels (the cube's rim) and covered tiles with hits — asserted from the
           oracle's image (a pixel is a hit when it differs from the same frame without the cube) and from rt_stats (k_beam walks
           fewer runs than the frame has tiles)
  sizes    70 x 45 (partial tiles at the right and the bottom edge) and 64 x 64; spp 1, 3, 4, 5, 8 (5 and 8: more than one sample group)
  shards   72 x 48 in bands of 8 rows (6 bands: shards of 2 and of 3) and 72 x 44 (5.5 bands: the last band is short), and bands of 4 rows,
           with which the coverage mask is off (no sky tiles: the path every frame took before)
  batch    K = 3 cameras, one of them looking away from the cube (every tile a sky tile)
  params   camera_records, pixel_beams, jitter_table, output_rgba8, dead_shadow_rays
  camera   three frames on one context, the camera turned so that tiles change from covered to sky and back: a marker or a colour
           left by an earlier frame must not reach a later one
  unknown  an object type the shader does not know (uniforms center_object_type 3; rt_set_instance_types admits 0..2 only): primary
           hits re-trace the unchanged ray from the camera until the bounce budget ends
  ring     three instances without camera records (the cfg5 path)"""
import os

import numpy as np
import pytest

from tests import scenes
from tests.exact import assert_frame_equals_oracle, quantize8
from vulkan_raytracing_amd import RtContext, host, tiling
from vulkan_raytracing_amd.api import INSTANCE_DTYPE

pytestmark = pytest.mark.gpu
RES = scenes.RES
CUBE = os.path.join(RES, "cube.obj")
OFF_CENTRE = (1.6, 0.7, 0.0)
CAMERA = (0.0, 0.0, 9.0)


@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


def translated(t):
    return np.array([1, 0, 0, t[0], 0, 1, 0, t[1], 0, 0, 1, t[2]], np.float32)


def turned(u, yaw_deg):
    """u with the camera turned about the up axis (default basis (1,0,0), (0,1,0), (0,0,-1))"""
    a = np.deg2rad(yaw_deg)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    v = u.copy()
    v[0]["right"][:3] = ry @ (1, 0, 0); v[0]["up"][:3] = ry @ (0, 1, 0); v[0]["forward"][:3] = ry @ (0, 0, -1)
    return v


def cube_scene(spp, ctx=None, max_bounce=2, obj_type=0, at=OFF_CENTRE):
    inst = [host.make_instance(translated(at), 0, 0)]
    u = host.default_uniforms(max_bounce_count=max_bounce, samples_per_pixel=spp, center_object_type=obj_type, orbiting_object_type=0)
    u[0]["position"][:3] = CAMERA
    return scenes.ScenePair([CUBE], inst, u, sky=scenes.synthetic_skybox(64), ctx=ctx)


def tile_kinds(ref, sky_only):
    """(sky tiles, tiles with hits and all-miss pixels, tiles with hits) of the oracle's frame: a pixel is a hit when the cube changes it"""
    hit = (ref.view(np.uint32) != sky_only.view(np.uint32)).any(axis=2)
    H, W = hit.shape
    n_sky = n_mixed = n_hit = 0
    for ty in range(0, H, 8):
        for tx in range(0, W, 8):
            t = hit[ty:ty + 8, tx:tx + 8]
            n_sky += int(not t.any()); n_hit += int(t.any()); n_mixed += int(t.any() and not t.all())
    return n_sky, n_mixed, n_hit


def assert_all_three_kinds(sp, W, H, ref, runs):
    sky_only, _ = cube_scene(int(sp.uniforms[0]["samples_per_pixel"]), at=(0.0, 0.0, 1000.0)).orc.render(W, H)   # the cube behind the camera
    n_sky, n_mixed, n_hit = tile_kinds(ref, sky_only)
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    assert n_hit >= 4 and n_mixed >= 4 and n_sky >= tiles // 2, (n_sky, n_mixed, n_hit)
    # k_beam walked one run per tile and sample group that has a traced sample: at least the tiles with hits, far fewer than all tiles
    groups = (int(sp.uniforms[0]["samples_per_pixel"]) + 3) // 4
    assert n_hit * groups <= runs <= (tiles - n_sky // 2) * groups, (runs, n_hit, n_sky, tiles)


def check(ctx, sp, W, H):
    gpu, st = ctx.trace(W, H)
    ref, rc = sp.orc.render(W, H)
    assert_frame_equals_oracle(gpu, sp.orc, W, H, ref=ref)
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == tuple(int(x) for x in rc)
    return gpu, ref


# ---- 1. odd frame sizes, sample counts on both sides of the workgroup's four ---------------------------------------------------

@pytest.mark.parametrize("spp", [1, 3, 4, 5, 8])
@pytest.mark.parametrize("W,H", [(70, 45), (64, 64)])
def test_frame_sizes_and_sample_counts(ctx, W, H, spp):
    sp = cube_scene(spp, ctx)
    gpu, ref = check(ctx, sp, W, H)
    counted, st = ctx.trace(W, H, counting=True)      # (the counting kernels: the same frame, and the number of runs k_beam walked)
    assert np.array_equal(counted.view(np.uint32), gpu.view(np.uint32))
    assert_all_three_kinds(sp, W, H, ref, int(st.tile_diag[2]))
    assert st.rays_shadow > 0


# ---- 2. shards -----------------------------------------------------------------------------------------------------------------

def render_shards(ctx, W, H, band, n):
    import torch
    rows_max = tiling.max_shard_rows(H, band, n)
    shards = []
    for s in range(n):
        buf = torch.zeros((max(rows_max, 1), W, 4), dtype=torch.float32, device="cuda:0")
        ctx.trace_shard(W, H, band, s, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
        ctx.synchronize()
        shards.append(buf.cpu().numpy()[:rows_max])
    return tiling.assemble(shards, H, W, band)


@pytest.mark.parametrize("W,H,band,n", [(72, 48, 8, 2), (72, 48, 8, 3), (72, 44, 8, 3), (72, 44, 8, 2), (72, 48, 8, 7), (72, 48, 4, 3)])
def test_shards_reassemble_to_the_oracles_frame(ctx, W, H, band, n):
    """bands of 8: whole tiles, the coverage mask is on (72 x 44: the last band is short; 7 shards of 6 bands: one shard is empty);
    bands of 4: the mask is off and no tile is a sky tile"""
    sp = cube_scene(4, ctx)
    full, ref = check(ctx, sp, W, H)
    out = render_shards(ctx, W, H, band, n)
    assert np.array_equal(out.view(np.uint32), full.view(np.uint32))
    assert_frame_equals_oracle(out, sp.orc, W, H, ref=ref)


# ---- 3. a frame batch, one of its cameras looking away -------------------------------------------------------------------------

@pytest.mark.parametrize("spp", [4, 5])
def test_batch_of_three_cameras(ctx, spp):
    import torch
    W, H = 70, 45
    sp = cube_scene(spp, ctx)
    frames = [turned(sp.uniforms, yaw) for yaw in (0.0, 120.0, -7.0)]      # frame 1 looks away: every tile a sky tile
    frames[2][0]["position"][:3] = (0.4, -0.3, 8.0)
    alone = []
    for u in frames:
        sp.set_uniforms(u)
        gpu, ref = check(ctx, sp, W, H)
        alone.append((gpu, ref))
    ctx.set_batch(np.stack([sp.instances] * 3), np.concatenate(frames))
    try:
        buf = torch.zeros((3, H, W, 4), dtype=torch.float32, device="cuda:0")
        ctx.trace_shard_batch(W, H, 8, 0, 1, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
        ctx.synchronize()
        out = buf.cpu().numpy()
    finally:
        ctx.set_instances(sp.instances); ctx.set_uniforms(frames[0])
    for k in range(3):
        assert np.array_equal(out[k].view(np.uint32), alone[k][0].view(np.uint32)), k
    # the frame that looks away shows the sky alone: the cube changes no pixel of it
    sky = cube_scene(spp, at=(0.0, 0.0, 1000.0))
    sky.set_uniforms(frames[1])
    assert np.array_equal(sky.orc.render(W, H)[0].view(np.uint32), out[1].view(np.uint32))


# ---- 4. parameters that choose another path through the same frame -------------------------------------------------------------

@pytest.mark.parametrize("name,value,default", [("camera_records", 0, 1), ("pixel_beams", 0, 1), ("jitter_table", 0, 1), ("output_rgba8", 1, 0),
                                                ("dead_shadow_rays", 0, 1)])
def test_parameter_matrix(ctx, name, value, default):
    W, H = 70, 45
    sp = cube_scene(4, ctx)
    base, ref = check(ctx, sp, W, H)
    ctx.set_param(name, value)
    try:
        img, st = ctx.trace(W, H)
    finally:
        ctx.set_param(name, default)
    if name == "output_rgba8":
        assert img.dtype == np.uint8 and np.array_equal(img, quantize8(base))
    else:
        assert np.array_equal(img.view(np.uint32), base.view(np.uint32))
    assert_frame_equals_oracle(img, sp.orc, W, H, ref=ref)
    again, _ = ctx.trace(W, H)
    assert np.array_equal(again.view(np.uint32), base.view(np.uint32))


# ---- 5. a camera that moves between the frames of one context ------------------------------------------------------------------

@pytest.mark.parametrize("spp", [4, 8])
def test_tiles_change_between_covered_and_sky(ctx, spp):
    W, H = 64, 64
    sp = cube_scene(spp, ctx)
    base = sp.uniforms.copy()
    refs = []
    for yaw in (0.0, 14.0, 0.0, -30.0, 14.0):      # the cube moves across the frame, out of it and back
        sp.set_uniforms(turned(base, yaw))
        gpu, ref = check(ctx, sp, W, H)
        refs.append(ref)
    assert (refs[0].view(np.uint32) != refs[1].view(np.uint32)).any(axis=2).sum() > 200      # the frames do differ
    assert np.array_equal(refs[0], refs[2]) and not np.array_equal(refs[1], refs[3])


# ---- 6. an object type the shader does not know, hit by primary rays -----------------------------------------------------------

def test_unknown_object_type_retraces_from_the_camera(ctx):
    W, H = 32, 32
    sp = cube_scene(2, ctx, max_bounce=3, obj_type=3, at=(0.5, 0.2, 0.0))
    gpu, ref = check(ctx, sp, W, H)
    st = ctx.stats()
    assert st.rays_secondary >= 3 * 20      # every primary hit is traced again at each of the three bounces
    ctx.set_param("pixel_beams", 0)
    try:
        per_ray, _ = ctx.trace(W, H)
    finally:
        ctx.set_param("pixel_beams", 1)
    assert np.array_equal(per_ray.view(np.uint32), gpu.view(np.uint32))


# ---- 7. several instances, no camera records (the cfg5 path) -------------------------------------------------------------------

def test_three_instances_without_camera_records(ctx):
    W, H = 64, 40
    inst = [host.make_instance(translated(t), 0, 0) for t in ((1.6, 0.7, 0.0), (-2.5, -0.5, -3.0), (0.2, 1.9, -6.0))]
    u = host.default_uniforms(max_bounce_count=2, samples_per_pixel=4, center_object_type=1, orbiting_object_type=0)
    u[0]["position"][:3] = CAMERA
    sp = scenes.ScenePair([CUBE], np.asarray(inst, INSTANCE_DTYPE), u, sky=scenes.synthetic_skybox(64), ctx=ctx)
    base, ref = check(ctx, sp, W, H)
    ctx.set_param("camera_records", 0)
    try:
        img, st = ctx.trace(W, H)
    finally:
        ctx.set_param("camera_records", 1)
    assert_frame_equals_oracle(img, sp.orc, W, H, ref=ref)
    assert st.rays_secondary > 0
