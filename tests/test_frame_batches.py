"""Frame batches (rt_set_batch + rt_trace_shard_batch, K <= 8 frames in one pass): EVERY per-frame field of a batch.

include/rt_api.h promises that the camera (position, right, up, forward), the light's position and its intensity may differ from
frame to frame and that the results are those of the K frames rendered one by one, bit for bit.  Each case below varies one of
those fields (or all of them), renders the frames one by one (rt_set_instances(update) + rt_set_uniforms + rt_trace_shard) and as
one batch, compares the images as bits and the ray counts as integers, and holds the frames of the K = 8 whole-frame batch to the
oracle's frames, one by one.  There is no tolerance anywhere in this file.

Frame: 104 x 60, spp 2.  60 rows are 7.5 bands of 8 and 3.75 bands of 16: the last band is short with both band heights, and the
shards (1 of 3 with bands of 8: bands 1, 4, 7; 1 of 2 with bands of 16: bands 1, 3) end in that short band.

Scenes (teapot.obj in the centre, cube.obj orbiting, tests/scenes.two_object_scene, synthetic 64-texel cube map):
  diffuse   centre diffuse, orbiter mirror, 2 bounces; the camera stands 10 in front so that the teapot fills a good part of the frame
            (the light matters on the diffuse branch only), the cube at the animation's time 0.2 beside it
  glass     centre glass, orbiter diffuse, 3 bounces: refracted paths end on the diffuse cube, so that k_tail shades with the light of
  mirror    centre mirror, orbiter diffuse, 3 bounces      the sample's own frame at bounces >= 1

What a refused call leaves behind (f): rt_set_batch compares the shared fields before it touches the context, so the context keeps
the state it had BEFORE the refused call — a single frame (rt_set_instances + rt_set_uniforms) still renders with rt_trace, a held
batch still renders with rt_trace_shard_batch.  rt_set_uniforms on a context that holds a batch is refused the same way (e)."""
import os

import numpy as np
import pytest

from tests import scenes
from tests.exact import assert_frame_equals_oracle
from vulkan_raytracing_amd import RtContext, host, tiling
from vulkan_raytracing_amd.api import INSTANCE_DTYPE, RtError

RES = scenes.RES
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
W, H, SPP = 104, 60, 2
# (K, band_rows, shard, n_shards)
SPLITS = ((2, 8, 0, 1), (8, 8, 0, 1), (3, 8, 1, 3), (5, 16, 1, 2))
INTENSITIES = (1.0, 0.0, 0.125, 0.25, 0.5, 2.0, 4.0, 8.0)      # frame 0 keeps the default; one is 0, three are larger than 1
NEAR = (0.0, 1.0, 10.0)                                        # the camera of the diffuse scene


@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_alt():
    """A context of librt_mi355x_alt.so: the product sources compiled with -DRT_ALT_KERNELS (k_packet among them)."""
    c = RtContext(0, variant="alt")
    yield c
    c.close()


# ---- scenes and frame lists (host side only) ----------------------------------------------------------------------------------

def make_scene(kind, ctx=None):
    center, orbit, bounces = {"diffuse": (0, 1, 2), "glass": (2, 0, 3), "mirror": (1, 0, 3)}[kind]
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), center, orbit, bounces, SPP,
                                 sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.2)
    if kind == "diffuse":
        u = sp.uniforms.copy(); u[0]["position"][:3] = NEAR
        sp.set_uniforms(u)
    return sp


def turned(u, yaw_deg, pitch_deg):
    """u with the camera basis turned by yaw (about up) and then pitch (about right): R = Ry(yaw) Rx(pitch) applied to the default
    basis (1,0,0), (0,1,0), (0,0,-1); orthonormal to float32 rounding"""
    a, b = np.deg2rad(yaw_deg), np.deg2rad(pitch_deg)
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    r = ry @ rx
    v = u.copy()
    v[0]["right"][:3] = r @ (1, 0, 0); v[0]["up"][:3] = r @ (0, 1, 0); v[0]["forward"][:3] = r @ (0, 0, -1)
    return v


def intensity_frames(sp, K=8):
    frames = []
    for k in range(K):
        u = sp.uniforms.copy(); u[0]["light_intensity"] = INTENSITIES[k]
        frames.append((sp.instances, u))
    return frames


# yaw, pitch in degrees from the default camera (0, 0, 20) looking down -z: the objects move across tile boundaries, frame 3 has the
# cube off screen and the teapot cut by the screen's edge, frame 4 looks away from everything (no object on screen)
TURNS = ((0.0, 0.0), (2.0, 0.0), (-3.5, 1.5), (23.0, -1.0), (60.0, 0.0), (-6.0, -4.0), (1.0, 5.5), (-11.0, 2.0))
ALL_MISS = 4


def orientation_frames(sp, K=8):
    base = sp.uniforms.copy(); base[0]["position"][:3] = (0.0, 0.0, 20.0)
    return [(sp.instances, turned(base, *TURNS[k])) for k in range(K)]


def animated_instances(k):
    anim = host.SceneAnimation()
    for j in range(k + 1):
        anim.animate(np.float32(0.2 + 0.07 * (j + 1)))
    return np.ascontiguousarray(anim.instances((0, 1)), INSTANCE_DTYPE)


def everything_frames(sp, K, first=0):
    """position, orientation, light position, intensity and the animated instances all differ per frame"""
    frames = []
    for k in range(first, first + K):
        inst = animated_instances(k)
        cube = inst["transform"][1][[3, 7, 11]]
        u = sp.uniforms.copy()
        u[0]["position"][:3] = (0.5 * cube[0] + 0.3 * k - 1.0, 0.5 + 0.25 * k, 14.0 - 0.3 * k)    # between the teapot and the cube: both on screen
        u = turned(u, 1.5 * k - 5.0, 1.0 - 0.6 * k)
        u[0]["light_position"][:3] = (5.0 - k, 5.0 + 0.5 * k, 5.0)
        u[0]["light_intensity"] = INTENSITIES[(k + 5) % 8]
        frames.append((inst, u))
    return frames


def oracle_frame(sp, inst, u):
    """the oracle's frame and ray counts for one (instances, uniforms); leaves the oracle in that state (sp.ctx is not touched)"""
    inst = np.ascontiguousarray(inst, INSTANCE_DTYPE)
    sp.orc.set_instances([inst[i].tobytes() for i in range(len(inst))])
    sp.orc.set_uniforms(u.tobytes())
    return sp.orc.render(W, H)


# ---- the two ways to render a list of (instances, uniforms) ----------------------------------------------------------------

def one_by_one(ctx, frames, band, shard, n):
    import torch
    rows = tiling.max_shard_rows(H, band, n)
    imgs, rays = [], np.zeros(3, np.int64)
    first = True
    for inst, u in frames:
        ctx.set_instances(inst, update=not first); first = False
        ctx.set_uniforms(u)
        buf = torch.zeros((rows, W, 4), dtype=torch.float32, device="cuda:0")
        ctx.trace_shard(W, H, band, shard, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
        st = ctx.stats()
        rays += (st.rays_primary, st.rays_secondary, st.rays_shadow)
        imgs.append(buf.cpu().numpy())
    return imgs, rays


def batched(ctx, frames, band, shard, n, update=False, set_batch=True):
    import torch
    rows = tiling.max_shard_rows(H, band, n)
    K = len(frames)
    if set_batch:
        ctx.set_batch(np.stack([f[0] for f in frames]), np.concatenate([f[1] for f in frames]), update=update)
    buf = torch.zeros((K, rows, W, 4), dtype=torch.float32, device="cuda:0")
    rows_real = ctx.shard_rows(H, band, shard, n)
    padded = (K + band + shard) % 2 == 1       # frame k's shard rows_max rows behind frame k - 1's (a padded buffer), or back to back
    ctx.trace_shard_batch(W, H, band, shard, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream,
                          frame_stride_bytes=rows * W * 16 if padded else 0)
    st = ctx.stats()
    out = buf.cpu().numpy()
    imgs = []
    for k in range(K):
        flat = out.reshape(-1, W, 4)
        first_row = k * (rows if padded else rows_real)
        img = np.zeros((rows, W, 4), np.float32); img[:rows_real] = flat[first_row:first_row + rows_real]
        imgs.append(img)
    return imgs, np.array([st.rays_primary, st.rays_secondary, st.rays_shadow], np.int64)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def check_both_ways(ctx, frames, band, shard, n, update=False, what=""):
    """the batch equals the frames one by one: images as bits, ray counts as integers.  Returns the batch's images and counts."""
    a_imgs, a_rays = one_by_one(ctx, frames, band, shard, n)
    b_imgs, b_rays = batched(ctx, frames, band, shard, n, update=update)
    rows_real = ctx.shard_rows(H, band, shard, n)
    assert rows_real > 0
    for k in range(len(frames)):
        bad = int((a_imgs[k][:rows_real].view(np.uint32) != b_imgs[k][:rows_real].view(np.uint32)).any(axis=2).sum())
        assert bad == 0, "%s K %d band %d shard %d/%d: frame %d differs from the frame rendered alone in %d pixels" % (what, len(frames), band, shard, n, k, bad)
    assert np.array_equal(a_rays, b_rays), (what, len(frames), band, shard, n, a_rays, b_rays)
    return b_imgs, b_rays


def check_batch_against_oracle(sp, frames, imgs, rays, which=None):
    """frames `which` (default: all) of a whole-frame batch equal the oracle's, and (all frames only) so do the summed ray counts"""
    total = np.zeros(3, np.int64)
    for k in (range(len(frames)) if which is None else which):
        ref, rc = oracle_frame(sp, *frames[k])
        try:
            assert_frame_equals_oracle(imgs[k][:H], sp.orc, W, H, ref=ref)
        except AssertionError as e:
            raise AssertionError("frame %d of the batch: %s" % (k, e)) from None
        total += rc.astype(np.int64)
    if which is None:
        assert np.array_equal(rays, total), (rays, total)


def back_to_single_frames(ctx, sp):
    ctx.set_instances(sp.instances)
    ctx.set_uniforms(sp.uniforms)


def oracle_frames_depend_on_intensity(sp):
    """the condition that keeps (a) honest: for every k >= 1 the oracle's frame k differs from the frame with frame 0's intensity"""
    frames = intensity_frames(sp)
    ref0, rc0 = oracle_frame(sp, *frames[0])
    assert rc0[2] > 0.15 * rc0[0]               # the diffuse teapot fills a good part of the frame: a shadow ray per diffuse hit
    refs = [ref0]
    for k in range(1, 8):
        ref, rc = oracle_frame(sp, *frames[k])
        differing = int((ref.view(np.uint32) != ref0.view(np.uint32)).any(axis=2).sum())
        assert differing > 0.1 * W * H, (k, differing)
        assert np.array_equal(rc, rc0)           # ... while the rays are the same: the intensity alone changes the frame
        refs.append(ref)
    for j in range(8):                           # and the eight values give eight different frames
        for k in range(j + 1, 8):
            assert not same_bits(refs[j], refs[k]), (j, k)


# ---- CPU: the honesty condition of (a), wherever the suite runs ---------------------------------------------------------------

def test_oracle_frames_depend_on_the_light_intensity():
    oracle_frames_depend_on_intensity(make_scene("diffuse"))


# ---- a. per-frame light intensity ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_light_intensity_is_the_frames_own(ctx):
    """The frames of a batch differ ONLY in light_intensity (eight values, 0 and values above 1 among them).  The batch equals the
    frames one by one for every split, and every frame of the K = 8 whole-frame batch equals the oracle's frame with that
    intensity; the oracle's frames are shown to depend on the intensity first."""
    sp = make_scene("diffuse", ctx)
    oracle_frames_depend_on_intensity(sp)
    try:
        for K, band, shard, n in SPLITS:
            frames = intensity_frames(sp, K)
            imgs, rays = check_both_ways(ctx, frames, band, shard, n, what="intensity")
            assert rays[2] > 0
            if (K, n) == (8, 1):
                check_batch_against_oracle(sp, frames, imgs, rays)
    finally:
        back_to_single_frames(ctx, sp)


# ---- b. per-frame camera orientation ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("off", [None, "primary_cover", "entry_points", "camera_records", "pixel_beams"])
def test_camera_orientation_is_the_frames_own(ctx, off):
    """The frames differ in right / up / forward (yaw and pitch of the default camera, position fixed): one coverage view and one
    entry-record view per frame.  Objects cross tile boundaries, leave the screen partly (frame 3) and entirely (frame 4: every
    tile's coverage is empty).  With the default parameters and with each of the four per-view mechanisms switched off."""
    sp = make_scene("diffuse", ctx)
    frames8 = orientation_frames(sp)
    counts = [oracle_frame(sp, *f)[1] for f in frames8]
    assert counts[ALL_MISS][1] == 0 and counts[ALL_MISS][2] == 0                     # nothing on screen: no bounce, no shadow ray
    assert counts[3][1] == 0 and 0.2 * counts[0][2] < counts[3][2] < 0.8 * counts[0][2]   # the cube off screen, the teapot partly
    for k in range(8):
        for c in ("right", "up", "forward"):
            assert abs(float(np.dot(frames8[k][1][0][c][:3].astype(np.float64), frames8[k][1][0][c][:3].astype(np.float64))) - 1.0) < 1e-6
        assert abs(float(np.dot(frames8[k][1][0]["right"][:3].astype(np.float64), frames8[k][1][0]["forward"][:3].astype(np.float64)))) < 1e-6
        assert abs(float(np.dot(frames8[k][1][0]["up"][:3].astype(np.float64), frames8[k][1][0]["forward"][:3].astype(np.float64)))) < 1e-6
    try:
        if off:
            ctx.set_param(off, 0)
        for K, band, shard, n in SPLITS:
            frames = frames8 if K == 8 else frames8[3:3 + K]     # (the partly visible and the empty frame are in every batch)
            imgs, rays = check_both_ways(ctx, frames, band, shard, n, what="orientation, %s off" % off)
            if (K, n) == (8, 1):
                check_batch_against_oracle(sp, frames, imgs, rays)
    finally:
        if off:
            ctx.set_param(off, 1)
        back_to_single_frames(ctx, sp)


# ---- c. everything at once ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["glass", "mirror"])
def test_every_field_differs_per_frame(ctx, kind):
    """Position, orientation, light position, intensity and the animated instances differ per frame; the centre object is glass or a
    mirror and the orbiter diffuse, 3 bounces, so that k_tail runs over all frames and shades with each frame's own light.  A first
    batch as a build (update = 0), then a second one on the same context as a refit (update = 1) of the first."""
    sp = make_scene(kind, ctx)
    try:
        for K, band, shard, n in SPLITS:
            frames = everything_frames(sp, K)
            imgs, rays = check_both_ways(ctx, frames, band, shard, n, update=False, what=kind)
            assert rays[1] > 0 and rays[2] > 0
            if (K, n) == (8, 1):
                check_batch_against_oracle(sp, frames, imgs, rays)
            frames2 = everything_frames(sp, K, first=2)
            a2, r2 = one_by_one(ctx, frames2, band, shard, n)
            batched(ctx, frames, band, shard, n, update=False)
            b2, q2 = batched(ctx, frames2, band, shard, n, update=True)
            rows_real = ctx.shard_rows(H, band, shard, n)
            for k in range(K):
                assert same_bits(a2[k][:rows_real], b2[k][:rows_real]), ("refit", kind, K, band, shard, n, k)
            assert np.array_equal(r2, q2)
    finally:
        back_to_single_frames(ctx, sp)


# ---- d. one far frame in a near batch -----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("far_at", [2, 0])
def test_one_far_frame_in_a_near_batch(ctx, far_at):
    """K = 4; one frame's camera stands 5000 away and looks at the scene, the others at the usual distance.  The far-frame decision
    is an OR over the frames of the batch, and the whole pass then runs without k_beam: the near frames must not change."""
    sp = make_scene("diffuse", ctx)
    near = []
    for k in range(3):
        u = sp.uniforms.copy(); u[0]["position"][:3] = (0.4 * k - 0.4, 1.0 + 0.2 * k, 10.0 + 0.5 * k)
        near.append((sp.instances, u))
    u = sp.uniforms.copy(); u[0]["position"][:3] = (0.0, 0.0, 5000.0)
    frames = near[:2] + [(sp.instances, u)] + near[2:]           # the far frame is frame 2 ...
    if far_at == 0:
        frames = [frames[2], frames[0], frames[1], frames[3]]     # ... or frame 0
    try:
        for band, shard, n in ((8, 0, 1), (8, 1, 3), (16, 1, 2)):
            imgs, rays = check_both_ways(ctx, frames, band, shard, n, what="far frame %d" % far_at)
            if n == 1:
                check_batch_against_oracle(sp, frames, imgs, rays, which=(1, 2) if far_at == 2 else (0, 1))   # the far frame and a near one
    finally:
        back_to_single_frames(ctx, sp)


# ---- e. rt_set_uniforms while a batch is held ---------------------------------------------------------------------------------

@pytest.mark.gpu
def test_set_uniforms_is_refused_while_a_batch_is_held(ctx):
    sp = make_scene("diffuse", ctx)
    frames = everything_frames(sp, 3)
    try:
        want, want_rays = batched(ctx, frames, 8, 0, 1)
        u = sp.uniforms.copy(); u[0]["samples_per_pixel"] = 1; u[0]["light_intensity"] = 3.0
        ctx.set_batch(np.stack([f[0] for f in frames]), np.concatenate([f[1] for f in frames]))
        with pytest.raises(RtError) as e:
            ctx.set_uniforms(u)
        assert e.value.code == RT_ERR_NOT_READY and "rt_set_batch" in str(e.value) and "rt_set_instances" in str(e.value)
        got, got_rays = batched(ctx, frames, 8, 0, 1, set_batch=False)        # exactly the batch as set
        for k in range(3):
            assert same_bits(got[k], want[k]), k
        assert np.array_equal(got_rays, want_rays)
        check_batch_against_oracle(sp, frames, got, got_rays)
        ctx.set_instances(frames[1][0])
        ctx.set_uniforms(u)                                                   # a single frame again: accepted
        img, st = ctx.trace(W, H)
        ref, rc = oracle_frame(sp, frames[1][0], u)
        assert_frame_equals_oracle(img, sp.orc, W, H, ref=ref)
        assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == tuple(int(x) for x in rc) and st.rays_primary == W * H
    finally:
        back_to_single_frames(ctx, sp)


# ---- f. shared-field validation ------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_shared_fields_are_validated_and_a_refused_batch_changes_nothing(ctx):
    sp = make_scene("diffuse", ctx)
    K = 3
    frames = everything_frames(sp, K)
    inst = np.stack([f[0] for f in frames])
    try:
        # the previous state is a single frame
        back_to_single_frames(ctx, sp)
        single, st0 = ctx.trace(W, H)
        for field, value in (("max_bounce_count", 3), ("samples_per_pixel", 1), ("center_object_type", 1), ("orbiting_object_type", 2)):
            us = [f[1].copy() for f in frames]
            assert us[K - 1][0][field] != value
            us[K - 1][0][field] = value
            with pytest.raises(RtError) as e:
                ctx.set_batch(inst, np.concatenate(us))
            assert e.value.code == RT_ERR_INVALID_ARGUMENT, field
            img, st = ctx.trace(W, H)
            assert same_bits(img, single) and st.rays_shadow == st0.rays_shadow, field
        # the previous state is a batch
        want, want_rays = batched(ctx, frames, 8, 1, 3)
        for field, value in (("max_bounce_count", 3), ("samples_per_pixel", 1), ("center_object_type", 1), ("orbiting_object_type", 2)):
            us = [f[1].copy() for f in frames]
            us[K - 1][0][field] = value
            with pytest.raises(RtError) as e:
                ctx.set_batch(inst, np.concatenate(us), update=True)
            assert e.value.code == RT_ERR_INVALID_ARGUMENT, field
            got, got_rays = batched(ctx, frames, 8, 1, 3, set_batch=False)
            for k in range(K):
                assert same_bits(got[k], want[k]), (field, k)
            assert np.array_equal(got_rays, want_rays)
        # the two informational offsets are not shared fields
        odd = []
        for k, (i, u) in enumerate(frames):
            v = u.copy()
            v[0]["orbiting_object_primitive_offset"] += 7 * k; v[0]["orbiting_object_vertex_offset"] += 11 * k
            odd.append((i, v))
        imgs, rays = check_both_ways(ctx, odd, 8, 0, 1, what="offset fields")
        check_batch_against_oracle(sp, odd, imgs, rays)
    finally:
        back_to_single_frames(ctx, sp)


# ---- g. the alt library with packet_trace 1 -----------------------------------------------------------------------------------

@pytest.mark.gpu
def test_alt_library_packet_trace_renders_a_batch_as_the_frames(ctx_alt):
    """k_packet starts every walk at frame 0's TLAS root, so the frames of a batch take the one-lane kernels whatever packet_trace
    says.  The teapot (and the camera with it) moves 9 units per frame: frame 2's teapot is nowhere near frame 0's, and a walk
    through frame 0's tree would miss it."""
    sp = make_scene("diffuse", ctx_alt)
    frames = []
    for k in range(3):
        inst = sp.instances.copy()
        inst["transform"][0][3] += 9.0 * k
        u = sp.uniforms.copy(); u[0]["position"][0] += 9.0 * k
        frames.append((inst, u))
    rc = [oracle_frame(sp, *f)[1] for f in frames]
    assert rc[2][2] > 0.15 * rc[2][0]                              # frame 2 sees its teapot
    try:
        a_imgs, a_rays = one_by_one(ctx_alt, frames, 8, 0, 1)      # packet_trace 0
        ctx_alt.set_param("packet_trace", 1)
        b_imgs, b_rays = batched(ctx_alt, frames, 8, 0, 1)
        for k in range(3):
            bad = int((a_imgs[k].view(np.uint32) != b_imgs[k].view(np.uint32)).any(axis=2).sum())
            assert bad == 0, "packet_trace 1: frame %d differs from the frame rendered alone in %d pixels" % (k, bad)
        assert np.array_equal(a_rays, b_rays)
        check_batch_against_oracle(sp, frames, b_imgs, b_rays, which=(2,))
    finally:
        ctx_alt.set_param("packet_trace", 0)
        back_to_single_frames(ctx_alt, sp)


# ---- h. through the multi-GPU host --------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_batches_through_the_multi_gpu_host(ctx):
    """rtm_set_batch on 3 logical devices (loopback): every assembled frame equals the single context's frame of the same batch, and
    rtm_set_uniforms on a slot that holds a batch reports rt_set_uniforms' refusal."""
    from vulkan_raytracing_amd import multi
    sp = make_scene("glass", ctx)
    frames = everything_frames(sp, 4)
    try:
        want, want_rays = batched(ctx, frames, 8, 0, 1)
    finally:
        back_to_single_frames(ctx, sp)
    m = multi.RtMulti([0, 0, 0], 2, loopback=True)
    try:
        g = sp.geom
        m.upload_geometry(g.verts, g.idx, g.ranges)
        m.set_instances(sp.instances); m.set_uniforms(sp.uniforms); m.set_skybox(sp.sky)
        m.set_batch(1, np.stack([f[0] for f in frames]), np.concatenate([f[1] for f in frames]))
        with pytest.raises(RtError) as e:
            m.set_uniforms(sp.uniforms, slot=1)
        assert e.value.code == RT_ERR_NOT_READY
        m.trace_async(1, W, H)
        img, st = m.trace_wait(1)
        assert img.shape == (4, H, W, 4)
        for k in range(4):
            bad = int((img[k].view(np.uint32) != want[k][:H].view(np.uint32)).any(axis=2).sum())
            assert bad == 0, "frame %d assembled from 3 devices differs from the single context's in %d pixels" % (k, bad)
        assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == tuple(int(x) for x in want_rays)
        m.set_instances(frames[0][0], slot=1)            # back to single frames: rtm_set_uniforms is accepted again
        m.set_uniforms(frames[0][1], slot=1)
        m.trace_async(1, W, H)
        one, _ = m.trace_wait(1)
        assert same_bits(one, want[0][:H])
    finally:
        m.close()
