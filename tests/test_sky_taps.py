"""The cube-map lookup fetches the two taps of a footprint row with ONE 8-byte load where the footprint lies inside a face (sample_sky,
csrc/kernels.hip); on a face edge it keeps its four single loads.  The texels and the arithmetic are the same, so frames stay those of
the oracle bit for bit.  The cameras here are aimed so that lookups fall on every face centre, on both sides of all 12 edges and on all
three faces around all 8 corners; the cube maps are small, so that one frame holds footprints with x0 even and odd, x0 = W - 2 (the
pair ends on its row's last texel) and y0 = H - 2 on layer 5 (the second pair ends on the LAST texel of the buffer: a load that reached
past it would read outside the allocation).  test_cameras_reach_every_footprint_class proves that from the oracle's own primary rays.

Cube sizes: 1x1 (every lookup touches a corner), 2x2, 3x3 (odd row stride: the two rows of a footprint differ in 8-byte alignment),
8x8, 5x4 (not a cube: per-face clamp), and no sky map at all.  spp 1, 2, 4 (a wave per sample) and 7 (the looped sky path).  The scene has
a mirror teapot, so misses are also shaded after a bounce (k_beam_shade, k_tail), and one case sends the same rays through
rt_shade_rays_device (k_ray_ingest)."""
import itertools
import os

import numpy as np
import pytest

from tests import exact, scenes
from tests.shade_reference import pinhole_rays
from vulkan_raytracing_amd import RtContext

RES = scenes.RES
TEAPOT, CUBE = os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj")
SIZES = {"1x1": (1, 1), "2x2": (2, 2), "3x3": (3, 3), "8x8": (8, 8), "5x4": (5, 4)}   # (W, H) of a face
SPPS = (1, 2, 4, 7)
FRAMES = ((32, 24), (40, 16))
MAX_BOUNCE = 2


def sky_faces(w, h, seed):
    """six random RGBA8 faces of h rows and w columns"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(6)]


def camera_towards(f, position=(0.0, 0.0, 20.0)):
    """(position, right, up, forward) of a camera looking along f, with the handedness of the default one (right x up = -forward)"""
    f = np.asarray(f, np.float64); f = f / np.linalg.norm(f)
    up0 = np.array([0.0, 0.0, 1.0]) if abs(f[1]) > 0.9 else np.array([0.0, 1.0, 0.0])
    r = np.cross(f, up0); r /= np.linalg.norm(r)
    return tuple(position), tuple(r), tuple(np.cross(r, f)), tuple(f)


def cameras():
    """the 26 directions of a cube's face centres (6), edge midpoints (12) and corners (8) from the default position, where (0, 0, -1)
    looks at the scene, and a close look at the mirror teapot, whose reflections spread over the whole cube map"""
    dirs = [d for d in itertools.product((-1, 0, 1), repeat=3) if any(d)]
    dirs.sort(key=lambda d: (sum(map(abs, d)), d))
    cams = [camera_towards(d) for d in dirs]
    cams.append(camera_towards((0.0, -0.1, -1.0), position=(0.0, 1.5, 7.0)))
    return cams


CAMERAS = cameras()


def frame_of(k):
    return FRAMES[k % 2]


def uniforms_for(sp, cam, spp):
    pos, right, up, fwd = cam
    u = sp.uniforms.copy()
    u[0]["position"][:3] = pos; u[0]["right"][:3] = right; u[0]["up"][:3] = up; u[0]["forward"][:3] = fwd
    u[0]["samples_per_pixel"] = spp
    return u


def make_scene(ctx=None, sky=None):
    return scenes.two_object_scene(TEAPOT, CUBE, 1, 0, MAX_BOUNCE, 1, sky=sky, ctx=ctx)   # mirror teapot, diffuse cube


def set_sky(sp, faces):
    sp.sky = faces
    sp.orc.set_skybox(faces)
    if sp.ctx is not None:
        sp.ctx.set_skybox(faces)


def footprints(d, W, H):
    """(layer, x0, y0) of the lookups of the miss directions d ((n, 3) float32), as sample_sky places them (float32 throughout)"""
    f32 = np.float32
    r = np.asarray(d, f32) * np.array([1, 1, -1], f32)
    a = np.abs(r)
    isz = (a[:, 2] >= a[:, 0]) & (a[:, 2] >= a[:, 1])
    isy = ~isz & (a[:, 1] >= a[:, 0])
    isx = ~isz & ~isy
    pos = np.where(isz, r[:, 2], np.where(isy, r[:, 1], r[:, 0])) >= 0
    layer = np.where(isz, 4, np.where(isy, 2, 0)) + np.where(pos, 0, 1)
    s = np.where(isz, np.where(pos, r[:, 0], -r[:, 0]), np.where(isy, r[:, 0], np.where(pos, -r[:, 2], r[:, 2])))
    t = np.where(isz, -r[:, 1], np.where(isy, np.where(pos, r[:, 2], -r[:, 2]), -r[:, 1]))
    ma = np.where(isz, a[:, 2], np.where(isy, a[:, 1], a[:, 0]))
    assert isx.sum() + isy.sum() + isz.sum() == len(r)
    u = f32(0.5) * (s / ma + f32(1)) * f32(W) - f32(0.5)
    v = f32(0.5) * (t / ma + f32(1)) * f32(H) - f32(0.5)
    x0 = np.clip(np.floor(u).astype(np.int64), -1, W - 1)
    y0 = np.clip(np.floor(v).astype(np.int64), -1, H - 1)
    return layer, x0, y0


def primary_miss_directions(orc, W, H):
    """the directions of the frame's primary rays (sample 0) that hit nothing: the ones that look the sky up"""
    rays = pinhole_rays(orc, W, H, 1)
    return rays[orc.intersect(rays)["inst"] < 0, 4:7]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", list(SIZES))
def test_cameras_reach_every_footprint_class(size):
    """the primary rays of the sky-only cameras (sample 0) place footprints on every face in every class: inside the face, beyond each
    of its four sides, beyond each of its four corners; inside a face with x0 even, x0 odd, x0 = W - 2, and y0 = H - 2 on layer 5"""
    W, H = SIZES[size]
    sp = make_scene()
    seen = set()
    for k, cam in enumerate(CAMERAS[:26]):
        sp.set_uniforms(uniforms_for(sp, cam, 1))
        fw, fh = frame_of(k)
        layer, x0, y0 = footprints(primary_miss_directions(sp.orc, fw, fh), W, H)
        seen |= set(zip(layer.tolist(), x0.tolist(), y0.tolist()))

    def classes(n):   # beyond the low side, inside (where the face has an inside), beyond the high side
        return [[-1], list(range(0, n - 1)), [n - 1]]

    for layer in range(6):
        for xs in classes(W):
            for ys in classes(H):
                if xs and ys:
                    assert any((layer, x, y) in seen for x in xs for y in ys), (size, layer, xs, ys)
    inside = {(l, x, y) for (l, x, y) in seen if 0 <= x < W - 1 and 0 <= y < H - 1}
    if W >= 2 and H >= 2:
        assert any(x % 2 == 0 for _, x, _ in inside) and any(x == W - 2 for _, x, _ in inside)
        assert any(l == 5 and y == H - 2 for l, _, y in inside)
        assert any(l == 5 and x == W - 2 and y == H - 2 for l, x, y in inside)   # the pair that ends on the buffer's last texel
    if W >= 3:
        assert any(x % 2 == 1 for _, x, _ in inside)
        # both alignments of a pair: texel index ((layer * H + y) * W + x) even and odd
        assert {((l * H + y) * W + x) % 2 for l, x, y in inside} == {0, 1}


def test_raygen_keeps_its_occupancy_and_uses_no_scratch():
    from tests.test_ray_query import _resource_usage
    found = [(name, r) for name, r in _resource_usage("resource-usage").items() if "k_raygen" in name]
    assert len(found) == 1, [n for n, _ in found]
    name, r = found[0]
    assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0, (name, r)
    assert int(r["Occupancy"]) >= 7, (name, r)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rig():
    c = RtContext(0)
    yield make_scene(ctx=c, sky=sky_faces(2, 2, 1))
    c.close()


def check_cameras(sp, spp, cams, bgra=False):
    hit = 0
    for k, cam in cams:
        sp.set_uniforms(uniforms_for(sp, cam, spp))
        W, H = frame_of(k)
        img, st = sp.ctx.trace(W, H)
        exact.assert_frame_equals_oracle(img, sp.orc, W, H, bgra=bgra)
        hit += int(st.rays_secondary)
    return hit


@pytest.mark.gpu
@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("size", list(SIZES))
def test_frames_equal_the_oracle(rig, size, spp):
    W, H = SIZES[size]
    set_sky(rig, sky_faces(W, H, seed=100 * W + H))
    bounced = check_cameras(rig, spp, list(enumerate(CAMERAS)))
    assert bounced > 0   # the mirror sent rays on: their misses were shaded after a bounce


@pytest.mark.gpu
@pytest.mark.parametrize("spp", (1, 4, 7))
def test_no_sky_map(spp):
    c = RtContext(0)
    try:
        sp = make_scene(ctx=c)
        check_cameras(sp, spp, [(k, CAMERAS[k]) for k in (0, 1, 5, 6, 18, 25, 26)])
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("param,bgra", [("output_rgba8", False), ("output_bgra8", True)])
def test_8bit_frames(param, bgra):
    """the finished pixels in the 8-bit formats (store_pixel's other store)"""
    c = RtContext(0)
    try:
        sp = make_scene(ctx=c, sky=sky_faces(3, 3, 5))
        c.set_param(param, 1)
        for spp in (2, 7):
            check_cameras(sp, spp, [(k, CAMERAS[k]) for k in (0, 1, 5, 6, 18, 25, 26)], bgra=bgra)
    finally:
        c.close()


@pytest.mark.gpu
def test_caller_rays_equal_the_oracle_frame(rig):
    """k_ray_ingest: every camera's primary rays (sample 0) as caller-generated rays; the points are the oracle's spp-1 frame"""
    import torch
    W, H = SIZES["3x3"]
    set_sky(rig, sky_faces(W, H, seed=33))
    for k, cam in enumerate(CAMERAS):
        rig.set_uniforms(uniforms_for(rig, cam, 1))
        fw, fh = frame_of(k)
        rays = torch.from_numpy(pinhole_rays(rig.orc, fw, fh, 1)).to("cuda:0")
        _, p = rig.ctx.shade_rays_device(rays, samples=1)
        torch.cuda.synchronize()
        exact.assert_frame_equals_oracle(p.cpu().numpy().reshape(fh, fw, 4), rig.orc, fw, fh)
