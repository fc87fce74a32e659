"""k_beam_shade fetches a pixel's surface once: the rows of a run (one row per sample of the run's 64 pixels) carry the fields of the
instance record and the three vertices of the last triangle from one row to the next (ShadeCarry, csrc/kernels.hip), a run whose hits
all lie in one instance reads that record once for the wave through the scalar cache (beam_body, csrc/kernels_beam.inc), and every
access of the epilogue goes through a global pointer.  Where the operands come from changed; the arithmetic did not — so every frame
here is, byte for byte, the frame of "fused_shade" 0 (k_beam + k_shade: the per-slot fetches of shade_slot without REG), with the same
ray counts and exactly one launch less (tests/test_fused_shade.py fused_and_two_launches), and one frame of every group is the oracle's
bit for bit.

Frames are 70 x 36: the last tile column (6 of 8 pixels) and the last tile row (4 of 8) are partial, so every frame has runs with dead
slots.  spp 1 .. 5: rows 1 .. 4 of a run, and at 5 a second sample group (a run of 64 and a run of 256 slots per tile).

  coarse     a cube a third of the frame wide: all samples of a pixel lie in one triangle, rows 1.. reuse everything row 0 fetched
  fine       a geodesic stand-in of 32 000 triangles about 40 pixels wide: the samples of most pixels hit different primitives of one
             instance — every row fetches a triangle again, and no row the instance
  straddle   the teapot in front of a large cube with sky around both: pixels on the teapot's silhouette have samples in two
             instances (the run is not instance-uniform, a lane changes instance between rows), pixels on the outer silhouettes have
             samples that miss inside a covered tile (the sky branch between two hits of one pixel)
  materials  a material table with its own exponents and types, over instances typed mirror, glass and diffuse; and over the
             two-way switch of the uniform block with the unknown type 3 for the centre object
  last       max_bounce_count 0 with a mirror: the `last` branch stores the ambient colour
"""
import os

import numpy as np
import pytest

from tests import scenes
from tests.test_fused_shade import CAMERA, CUBE, check_oracle, full_frame, fused_and_two_launches, translated
from vulkan_raytracing_amd import RtContext, host
from vulkan_raytracing_amd.api import INSTANCE_DTYPE, MATERIAL_DTYPE, MATERIAL_TYPE_OF_INSTANCE

W, H = 70, 36
SPP = [1, 2, 3, 4, 5]
TEAPOT = os.path.join(scenes.RES, "teapot.obj")


@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    c.set_timing(1)
    yield c
    c.close()


def scene(ctx, paths, placed, spp, max_bounce=2, center_type=0, orbiting_type=0):
    """placed: (transform, customIndex, mesh) per instance"""
    inst = [host.make_instance(t, k, m) for t, k, m in placed]
    u = host.default_uniforms(max_bounce_count=max_bounce, samples_per_pixel=spp, center_object_type=center_type, orbiting_object_type=orbiting_type)
    u[0]["position"][:3] = CAMERA
    return scenes.ScenePair(paths, np.asarray(inst, INSTANCE_DTYPE), u, sky=scenes.synthetic_skybox(64), ctx=ctx)


def both_ways(ctx, sp, oracle_too):
    img, rays = fused_and_two_launches(ctx, lambda: full_frame(ctx, W, H))
    if oracle_too:
        check_oracle(sp, img, rays, W, H)
    return img, rays


@pytest.mark.gpu
@pytest.mark.parametrize("spp", SPP)
def test_coarse_mesh_rows_reuse_one_triangle(ctx, spp):
    sp = scene(ctx, [CUBE], [(translated((0.4, 0.1, 3.0), 1.5), 0, 0)], spp)
    img, rays = both_ways(ctx, sp, spp == 4)
    assert rays[2] > 200 * spp          # the cube fills hundreds of pixels: diffuse hits with shadow rays


@pytest.mark.gpu
@pytest.mark.parametrize("spp", SPP)
def test_sub_pixel_triangles_every_row_fetches(ctx, spp):
    mesh, _ = host.armadillo_path(scenes.RES, frequency=40)
    sp = scene(ctx, [mesh], [(translated((0.3, -0.2, 0.0)), 0, 0)], spp)
    n_tris = len(sp.geom.idx) // 3
    img, rays = both_ways(ctx, sp, spp == 3)
    # the half of the mesh that faces the camera has several triangles for every pixel it covers (rays_shadow: one per diffuse hit)
    assert rays[2] > 0 and n_tris // 2 > 4 * (rays[2] // spp)


@pytest.mark.gpu
@pytest.mark.parametrize("spp", SPP)
def test_pixels_straddling_two_instances_and_the_sky(ctx, spp):
    sp = scene(ctx, [TEAPOT, CUBE], [(translated((0.3, -0.7, 2.0)), 0, 0), (translated((1.2, 0.2, -2.5), 2.2), 1, 1)], spp)
    img, rays = both_ways(ctx, sp, spp == 4)
    assert 0 < rays[2] < rays[0]                  # (hits, and sky around them)


MATERIALS = np.zeros(4, MATERIAL_DTYPE)
MATERIALS[0] = ((0.1, 0.2, 0.3), 12.0, (0.9, 0.3, 0.5), 1.3, (0.2, 0.2, 0.2), MATERIAL_TYPE_OF_INSTANCE)
MATERIALS[1] = ((0.3, 0.1, 0.1), 50.0, (0.3, 0.8, 0.5), 1.5, (0.6, 0.6, 0.6), 0)
MATERIALS[2] = ((0.2, 0.2, 0.2), 10.0, (0.5, 0.5, 0.5), 1.7, (0.2, 0.2, 0.2), 1)
MATERIALS[3] = ((0.05, 0.3, 0.2), 3.0, (0.1, 0.9, 0.9), 1.1, (0.9, 0.9, 0.9), 2)
THREE_CUBES = [(translated((-2.1, 0.3, 1.0)), 0, 0), (translated((0.2, -0.2, 2.0)), 1, 0), (translated((2.3, 0.4, 0.5)), 1, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("types", [(1, 2, 0), None], ids=["instance_types", "unknown_type_of_the_uniform_block"])
@pytest.mark.parametrize("spp", SPP)
def test_material_table_and_instance_types(ctx, spp, types):
    # without instance types: customIndex 0 is of the unknown type 3 (re-traced from the camera), the others are mirrors
    sp = scene(ctx, [CUBE], THREE_CUBES, spp, center_type=3, orbiting_type=1)
    n_prims = len(sp.geom.idx) // 3
    sp.set_instance_types(types)
    # material 0 (every fifth primitive or so) leaves the type to the instance; 1, 2, 3 are diffuse, mirror and glass themselves
    sp.set_materials(MATERIALS, ((np.arange(n_prims) * 7 // 5) % 4).astype(np.uint32))
    try:
        img, rays = both_ways(ctx, sp, spp == 4)
        assert rays[1] > 0 and rays[2] > 0
    finally:
        ctx.set_materials(None)
        ctx.set_instance_types(None)


@pytest.mark.gpu
@pytest.mark.parametrize("spp", SPP)
def test_no_bounce_budget_in_partial_tiles(ctx, spp):
    # a mirror that reaches into the partial last tile column and row, and no bounce: every hit takes the `last` branch
    sp = scene(ctx, [CUBE, CUBE], [(translated((2.6, -1.3, 3.0), 1.4), 0, 0), (translated((-1.5, 0.5, 0.0)), 1, 1)], spp, max_bounce=0, center_type=1)
    img, rays = both_ways(ctx, sp, spp == 4)
    assert rays[1] == 0 and rays[2] > 0
    # the frame's last column and last row are not background only: the mirror covers pixels of the partial tiles
    flat = np.asarray(img).reshape(H, W, -1)
    ambient = np.array([0.08, 0.24, 0.08], np.float32)
    is_ambient = np.all(np.isclose(flat[..., :3], ambient, atol=1e-6), axis=-1)
    assert is_ambient[:, 64:].any() and is_ambient[32:, :].any()
