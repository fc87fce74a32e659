"""The exact frame and hit-record comparisons of tests/exact.py (CPU only)."""
import os

import numpy as np
import pytest

from oracle import ingest, oracle
from tests import exact, scenes

W, H = 48, 40


def frame(seed=3):
    rng = np.random.default_rng(seed)
    img = rng.random((H, W, 4), dtype=np.float32)
    img[..., 3] = 1.0
    return img


class NoOracle:
    """stands in for the oracle where the frames are made up: brute force 'renders' the given frame"""

    def __init__(self, img):
        self.img = img

    def render_pixels(self, W, H, xy, use_bvh=True):
        assert not use_bvh
        return self.img[xy[:, 1], xy[:, 0]]


def test_identical_frames_pass():
    a = frame()
    assert exact.assert_frame_equals_oracle(a.copy(), NoOracle(a), W, H, ref=a) is not None
    assert exact.assert_frame_equals_oracle(a.copy(), NoOracle(a), W, H, y0=5, y1=9, ref=a) is not None


def test_one_ulp_fails():
    a = frame()
    g = a.copy()
    g[7, 11, 1] = np.nextafter(g[7, 11, 1], np.float32(2.0))
    with pytest.raises(AssertionError) as e:
        exact.assert_frame_equals_oracle(g, NoOracle(a), W, H, ref=a)
    msg = str(e.value)
    assert msg.startswith("1 of %d pixels" % (W * H)) and "(x 11, y 7)" in msg
    assert "the GPU agrees on 0, the oracle's BVH mode on 1" in msg
    # outside the band that is compared the difference does not count; inside it does
    exact.assert_frame_equals_oracle(g, NoOracle(a), W, H, y0=0, y1=7, ref=a)
    exact.assert_frame_equals_oracle(g, NoOracle(a), W, H, y0=8, y1=H, ref=a)
    with pytest.raises(AssertionError):
        exact.assert_frame_equals_oracle(g, NoOracle(a), W, H, y0=7, y1=8, ref=a)


def test_signed_zero_fails():
    a = frame()
    a[3, 4, 0] = 0.0
    g = a.copy()
    g[3, 4, 0] = -0.0
    assert np.abs(g - a).max() == 0.0                 # what a max-abs bar sees
    with pytest.raises(AssertionError) as e:
        exact.assert_frame_equals_oracle(g, NoOracle(a), W, H, ref=a)
    assert "(x 4, y 3)" in str(e.value)


def test_nan_pixel_fails():
    a = frame()
    g = a.copy()
    g[H - 1, W - 1, 2] = np.nan
    with pytest.raises(AssertionError) as e:
        exact.assert_frame_equals_oracle(g, NoOracle(a), W, H, ref=a)
    assert "(x %d, y %d)" % (W - 1, H - 1) in str(e.value) and "NaN" in str(e.value)
    # NaN on both sides with the same bits is equal; with other payload bits it is not
    a[0, 0, 0] = g[0, 0, 0] = np.nan
    g[H - 1, W - 1, 2] = a[H - 1, W - 1, 2]
    exact.assert_frame_equals_oracle(g, NoOracle(a), W, H, ref=a)
    g[0, 0, 0] = np.uint32(0x7FC00001).view(np.float32)
    with pytest.raises(AssertionError):
        exact.assert_frame_equals_oracle(g, NoOracle(a), W, H, ref=a)


@pytest.mark.parametrize("bgra", [False, True])
def test_uint8_frames(bgra):
    a = frame()
    a[2, 2, :3] = (1.5, -0.25, 0.5)                   # clamped on both ends, 0.5 * 255 + 0.5 = 128
    g = exact.quantize8(a, bgra)
    assert g.dtype == np.uint8 and g.shape == (H, W, 4)
    assert g[2, 2].tolist() == ([128, 0, 255, 255] if bgra else [255, 0, 128, 255])
    exact.assert_frame_equals_oracle(g, NoOracle(a), W, H, ref=a, bgra=bgra)
    with pytest.raises(AssertionError):
        exact.assert_frame_equals_oracle(g, NoOracle(a), W, H, ref=a, bgra=not bgra)
    g[9, 1, 3] ^= 1
    with pytest.raises(AssertionError) as e:
        exact.assert_frame_equals_oracle(g, NoOracle(a), W, H, ref=a, bgra=bgra)
    assert str(e.value).startswith("1 of") and "(x 1, y 9)" in str(e.value) and "oracle's BVH mode on 1" in str(e.value)


def cube_scene():
    """BASELINE config 1 (tests/test_oracle.py): cube_scene.obj, depth 1, spp 1"""
    inst = [ingest.pack_instance(ingest.glm_to_vulkan(ingest.mat_identity()), 0, mesh=0)]
    u = np.frombuffer(ingest.pack_uniforms(max_bounce=0, spp=1, center_type=0, orbit_type=0), dtype=np.uint8)
    sa = ingest.SceneArrays([os.path.join(scenes.RES, "cube_scene.obj")])
    S = oracle.OracleScene()
    S.set_geometry(sa.verts, sa.idx, sa.ranges)
    S.set_instances(inst)
    S.set_uniforms(u.tobytes())
    S.set_skybox(scenes.synthetic_skybox(32))
    return S


def test_a_real_oracle_scene_names_the_altered_pixel_and_sides_with_the_oracle():
    S = cube_scene()
    Wc, Hc = 64, 48
    ref, _ = S.render(Wc, Hc)
    assert exact.assert_frame_equals_oracle(ref.copy(), S, Wc, Hc) is not None     # renders the reference itself
    lit = np.argwhere(np.abs(ref[..., :3] - ref[0, 0, :3]).max(axis=2) > 0)     # a pixel that is not sky-coloured like the corner
    y, x = (int(v) for v in lit[len(lit) // 2])
    g = ref.copy()
    g[y, x, 1] = np.nextafter(g[y, x, 1], np.float32(0.0))
    with pytest.raises(AssertionError) as e:
        exact.assert_frame_equals_oracle(g, S, Wc, Hc, ref=ref)
    msg = str(e.value)
    assert msg.startswith("1 of %d pixels" % (Wc * Hc)), msg
    assert "(x %d, y %d) gpu" % (x, y) in msg
    assert "the GPU agrees on 0, the oracle's BVH mode on 1, neither on 0" in msg
    assert "(x %d, y %d) brute force" % (x, y) in msg and "sides with oracle BVH" in msg
    # a band that holds the pixel fails, one that does not passes
    with pytest.raises(AssertionError):
        exact.assert_frame_equals_oracle(g, S, Wc, Hc, y0=y, y1=y + 1)
    exact.assert_frame_equals_oracle(g, S, Wc, Hc, y0=0, y1=y, ref=ref)


def test_hit_records_compare_every_field_as_bits():
    S = cube_scene()
    rays = scenes.random_rays(400, seed=4, target_radius=5.0)
    o = S.intersect(rays)
    assert (o["inst"] >= 0).any()
    exact.assert_hits_equal_oracle(o.copy(), S, rays, ref=o)
    k = int(np.nonzero(o["inst"] >= 0)[0][0])
    for field in ("t", "u", "v", "prim", "inst"):
        g = o.copy()
        if field in ("prim", "inst"):
            g[field][k] += 1
        else:
            g[field][k] = np.nextafter(g[field][k], np.float32(np.inf))
        with pytest.raises(AssertionError) as e:
            exact.assert_hits_equal_oracle(g, S, rays)
        msg = str(e.value)
        assert msg.startswith("1 of 400 hit records") and ("ray %d:" % k) in msg, (field, msg)
        assert "the GPU agrees on 0, the oracle's BVH mode on 1" in msg, (field, msg)
