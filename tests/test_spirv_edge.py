"""The shading path against the reference's own compiled shaders on the cases the reference never ships.

tests/golden/spirv_fixtures_edge.npz (made by tests/golden/make_spirv_fixtures.py --set edge) holds what the interpreted shader.rgen.spv /
shader.rchit.spv / miss modules computed on sixteen small scenes: sheared, mirrored and anisotropic instance transforms, the camera and the
light inside a mesh, object types outside 0..2, spp 2, 3, 5, 7 and 16, lightIntensity 0 and 3.5, a rolled camera whose basis is neither
unit nor orthogonal, a ring of seven instances.  The CPU tests hold the oracle to the records (and check that the records can tell a
wrong normal from a right one); the GPU tests hold the kernels to the oracle bit for bit and to the records at the same bars.

Every scene has the teapot and the cube with custom index == mesh (src/shader.rchit:52 takes the vertex offsets from the custom index, the
product takes them from the mesh: custom indices that do not follow the mesh are a product extension and not part of this set)."""
import json
import os

import numpy as np
import pytest

from oracle import oracle
from tests import scenes
from tests.exact import assert_frame_equals_oracle
from tests.shade_reference import average_points, shade_samples
from tests.spirv_replay import AMBIENT, SPV_TOL, SPV_TOL_LIT, replay_records
from vulkan_raytracing_amd import host

GOLD = os.path.join(scenes.ROOT, "tests", "golden")
KEYS = [m["key"] for m in json.load(open(os.path.join(GOLD, "spirv_fixtures_edge.json")))["scenes"]]
PIXEL_TOL, PIXEL_SHARE = 2e-4, 0.995     # the bar of test_oracle.py's pixel test; here for per-sample colours too (see the sample test)


class EdgeRig:
    """The edge scenes and ONE oracle scene for all of them: they share the meshes and the cube map (decoded once per module), and
    differ in instances and uniforms only."""

    def __init__(self):
        self.scenes = {sc.key: sc for sc in scenes.load_spirv_fixtures("edge")}
        first = next(iter(self.scenes.values()))
        assert all(sc.paths == first.paths and sc.sky_dir == first.sky_dir for sc in self.scenes.values())
        self.geom = first.geometry
        self.sky = host.load_skybox(first.sky_dir)
        self.orc = oracle.OracleScene()
        self.orc.set_geometry(self.geom.verts, self.geom.idx, self.geom.ranges)
        self.orc.set_skybox(self.sky)
        self.current = None
        self._cache = {}

    def select(self, key):
        sc = self.scenes[key]
        if self.current != key:
            self.orc.set_instances([sc.instances[i].tobytes() for i in range(len(sc.instances))])
            self.orc.set_uniforms(sc.uniforms.tobytes())
            self.current = key
        return sc

    def oracle_of(self, sc):
        self.select(sc.key)
        return self.orc

    def cached(self, what, key, make):
        if (what, key) not in self._cache:
            self._cache[(what, key)] = make()
        return self._cache[(what, key)]

    # -- per scene, computed once and shared between the tests (read-only) ---------------------------------------------------------
    def spp(self, key):
        return int(self.scenes[key].uniforms[0]["samples_per_pixel"])

    def max_bounce(self, key):
        return int(self.scenes[key].uniforms[0]["max_bounce_count"])

    def recorded_samples(self, key):
        """(bounce-0 records, last == 1 records) of the scene, each sample-major: row i * P + p is sample i of recorded pixel p"""
        def make():
            sc = self.scenes[key]
            b, spp, P = sc.bounces, self.spp(key), len(sc.pixels)
            slot = {(int(p["px"]), int(p["py"])): k for k, p in enumerate(sc.pixels)}
            out = []
            for sel in (b["bounce"] == 0, b["last"] == 1):
                r = b[sel]
                pos = np.array([int(x["sample"]) * P + slot[(int(x["px"]), int(x["py"]))] for x in r])
                assert len(r) == spp * P and np.array_equal(np.sort(pos), np.arange(spp * P))    # one per sample of every pixel
                out.append(r[np.argsort(pos)])
            return out
        return self.cached("samples", key, make)

    def oracle_frame(self, key):
        def make():
            sc = self.select(key)
            return self.orc.render(sc.width, sc.height)
        return self.cached("frame", key, make)

    def oracle_samples_of_recorded_rays(self, key):
        """shade_reference on the RECORDED bounce-0 rays (what rt_shade_rays_device is given)"""
        def make():
            sc = self.select(key)
            first, _ = self.recorded_samples(key)
            return shade_samples(self.orc, record_rays(first["o"], first["d"]), len(sc.pixels), self.max_bounce(key))
        return self.cached("shade", key, make)


def record_rays(o, d, tmax=10000.0):
    rays = np.zeros((len(o), 8), np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 0.001, d, tmax
    return rays


@pytest.fixture(scope="module")
def rig():
    return EdgeRig()


def linear_parts(sc):
    return [np.asarray(i["transform"], np.float64).reshape(3, 4)[:, 0:3] for i in sc.instances]


def types_of(sc, b):
    """the object type of every hit record (src/shader.rgen:96)"""
    u = sc.uniforms[0]
    return np.where(b["object_index"] == 0, int(u["center_object_type"]), int(u["orbiting_object_type"]))


def dot(a, b):
    return np.einsum("ij,ij->i", np.asarray(a, np.float64), np.asarray(b, np.float64))


def object_normals(rig, sc, b):
    """the interpolated object-space normal of every hit record (src/shader.rchit:62-91), in binary64"""
    v = np.asarray(rig.geom.verts, np.float64).reshape(-1, 6)
    idx = np.asarray(rig.geom.idx, np.int64)
    n = np.zeros((len(b), 3))
    for k, r in enumerate(b):
        first_float, first_index, _ = rig.geom.ranges[int(sc.instances[int(r["inst"])]["mesh"])]
        a, bb, c = v[first_float // 6 + idx[first_index + 3 * int(r["prim"]):first_index + 3 * int(r["prim"]) + 3], 3:6]
        n[k] = a * (1.0 - float(r["u"]) - float(r["v"])) + bb * float(r["u"]) + c * float(r["v"])
    return n


def unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


# ---- coverage: every scene holds the branch it is named for --------------------------------------------------------------------------------

def test_edge_set_is_the_committed_one(rig):
    assert list(rig.scenes) == KEYS and len(KEYS) == 16
    assert os.path.getsize(os.path.join(GOLD, "spirv_fixtures_edge.npz")) <= os.path.getsize(os.path.join(GOLD, "spirv_fixtures.npz"))
    for sc in rig.scenes.values():
        assert 37 <= sc.width <= 96 and 23 <= sc.height <= 54
        assert [os.path.basename(p) for p in sc.paths] == ["teapot.obj", "cube.obj"]
        assert all((int(i["custom_index_and_mask"]) & 0xFFFFFF) == int(i["mesh"]) for i in sc.instances)    # the reference's convention
        assert np.all(sc.pixels["rgba"][:, 3] == 1.0)
    whole = [k for k, sc in rig.scenes.items() if len(sc.pixels) == sc.width * sc.height]
    assert whole == ["sheared_mirrored_glass_cube", "inside_diffuse"]
    spps = sorted({rig.spp(k) for k in KEYS})
    assert spps == [1, 2, 3, 5, 7, 16]


def test_every_edge_scene_contains_the_branch_it_is_named_for(rig):
    """Minimum counts; in brackets what the generator recorded."""
    S = rig.scenes

    def parts(key):
        sc = S[key]
        b = sc.bounces
        hit = b["inst"] >= 0
        return sc, b, hit, dot(b["d"], b["N"]), b["last"] == 0

    def on_negative_det(sc, b, hit):
        neg = [k for k, L in enumerate(linear_parts(sc)) if np.linalg.det(L) < 0]
        return neg, hit & np.isin(b["inst"], neg)

    # the sheared scenes: hits on the instance with det < 0, outwards hits and total internal reflection inside it
    for key, inst, n_hits, n_tir in (("sheared_mirrored_glass", 0, 600, 200), ("sheared_mirrored_glass_cube", 1, 1300, 600)):   # [660 hits, 247 TIR], [1395, 643]
        sc, b, hit, nd, cont = parts(key)
        neg, on = on_negative_det(sc, b, hit)
        assert neg == [inst] and on.sum() >= n_hits, (key, on.sum())
        tir = on & (nd > 0) & cont & (dot(b["nd"], b["N"]) < 0)         # left the surface on the side it came from
        assert tir.sum() >= n_tir and (on & (nd > 0)).sum() >= n_tir and (on & (nd < 0)).sum() >= 200, key
        assert b["sample"].max() == rig.spp(key) - 1 and b["bounce"].max() == rig.max_bounce(key)
    assert (S["sheared_mirrored_glass_cube"].width, S["sheared_mirrored_glass_cube"].height) == (37, 23)
    assert rig.spp("sheared_mirrored_glass") == 7 and rig.max_bounce("sheared_mirrored_glass") == 5 and rig.max_bounce("sheared_mirrored_glass_cube") == 6
    # anisotropic (1e-2, 1, 3): lit and shadowed hits on the scaled teapot                                              [166 hits, 91 lit in all]
    sc, b, hit, nd, cont = parts("anisotropic_diffuse")
    s = np.linalg.svd(linear_parts(sc)[0], compute_uv=False)
    assert np.allclose(s, [3.0, 1.0, 1e-2], rtol=1e-6)
    assert (hit & (b["inst"] == 0) & (b["shadow"] == 1)).sum() >= 150 and ((b["shadow"] == 1) & (b["occluded"] == 0)).sum() >= 80
    # the camera inside the teapot
    for key in ("inside_glass", "inside_diffuse", "inside_mirror"):
        assert tuple(S[key].uniforms[0]["position"][:3]) == (0.0, np.float32(0.9), 0.0)
    sc, b, hit, nd, cont = parts("inside_glass")                          # [827 outwards hits, 302 of them totally reflected, deepest bounce 8]
    assert (hit & (nd > 0)).sum() >= 800 and (hit & (nd > 0) & cont & (dot(b["nd"], b["N"]) < 0)).sum() >= 300
    assert rig.spp("inside_glass") == 3 and rig.max_bounce("inside_glass") == 8 and b["bounce"].max() == 8
    sc, b, hit, nd, cont = parts("inside_diffuse")                        # [1296 of 1296]
    first = b["bounce"] == 0
    assert first.all() and hit.all() and len(b) == sc.width * sc.height and np.all(b["inst"] == 0)
    assert np.all(b["shadow"] == 0) and np.all(b["last"] == 1) and np.all(b["color"] == AMBIENT) and np.all(nd >= 0)
    sc, b, hit, nd, cont = parts("inside_mirror")                         # [122 primary hits from inside, all reflected]
    first = b["bounce"] == 0
    assert rig.max_bounce("inside_mirror") == 9 and (first & hit & (nd > 0) & cont).sum() >= 120
    # unknown types: the loop goes on with the ray it traced, until the budget ends                                    [198, 66]
    sc, b, hit, nd, cont = parts("unknown_types")
    u = sc.uniforms[0]
    assert (int(u["center_object_type"]), int(u["orbiting_object_type"]), int(u["max_bounce_count"])) == (3, 7, 3)
    same = (b["no"].view(np.uint32) == b["o"].view(np.uint32)).all(1) & (b["nd"].view(np.uint32) == b["d"].view(np.uint32)).all(1)
    assert np.array_equal(cont, hit & (b["bounce"] < 3)) and np.all(same[cont]) and cont.sum() >= 190
    ended = hit & (b["last"] == 1)
    assert ended.sum() >= 60 and np.all(b["bounce"][ended] == 3) and np.all(b["color"][ended] == AMBIENT)
    assert (hit & (b["object_index"] == 0)).sum() >= 100 and (hit & (b["object_index"] == 1)).sum() >= 100
    # lights
    sc, b, hit, nd, cont = parts("light_inside")                          # [116 shadow rays, all occluded: the teapot's own wall]
    assert tuple(sc.uniforms[0]["light_position"]) == (0.0, np.float32(0.9), 0.0)
    assert (b["shadow"] == 1).sum() >= 100 and np.all(b["occluded"][b["shadow"] == 1] == 1)
    sc, b, hit, nd, cont = parts("light_close")                           # [35 shadow rays with tmax < 0.5, all lit, the shortest 0.141; the light is 0.1 from the face]
    near = (b["shadow"] == 1) & (b["stmax"] < 0.5)
    assert near.sum() >= 30 and b["stmax"][near].min() < 0.15 and (near & (b["occluded"] == 0)).sum() >= 30
    sc0, b0, _, _, _ = parts("intensity_0")                               # [44 lit]
    lit = (b0["shadow"] == 1) & (b0["occluded"] == 0)
    assert float(sc0.uniforms[0]["light_intensity"]) == 0.0 and lit.sum() >= 40 and np.all(b0["color"][lit] == AMBIENT)
    sc1, b1, _, _, _ = parts("intensity_3p5")                             # [40 lit, the brightest channel 5.8]
    lit = (b1["shadow"] == 1) & (b1["occluded"] == 0)
    assert float(sc1.uniforms[0]["light_intensity"]) == 3.5 and lit.sum() >= 35 and b1["color"][lit].max() > 3.5
    # depths and sample counts
    sc, b, hit, nd, cont = parts("depth0_spp1")                           # [61 hits, each the end of its path]
    assert rig.max_bounce("depth0_spp1") == 0 and rig.spp("depth0_spp1") == 1 and b["bounce"].max() == 0 and b["sample"].max() == 0
    assert hit.sum() >= 55 and np.all(b["last"] == 1) and np.all(b["color"][hit] == AMBIENT) and set(types_of(sc, b[hit])) == {1, 2}
    sc, b, hit, nd, cont = parts("spp5")
    assert b["sample"].max() == 4 and (b["sample"] == 4).sum() >= 140          # [154 records of sample 4]
    sc, b, hit, nd, cont = parts("spp16")                                 # [273 lit samples, 205 of them of samples 4..15, 15 of sample 15]
    lit = (b["shadow"] == 1) & (b["occluded"] == 0)
    assert b["sample"].max() == 15 and lit.sum() >= 250 and (lit & (b["sample"] > 3)).sum() >= 180 and (lit & (b["sample"] == 15)).sum() >= 10
    # the camera: rolled, not unit, not orthogonal
    u = S["rolled_anamorphic_camera"].uniforms[0]
    r, up, f = (np.asarray(u[k][:3], np.float64) for k in ("right", "up", "forward"))
    lengths = [np.linalg.norm(x) for x in (r, up, f)]
    assert min(abs(l - 1.0) for l in lengths) > 0.15 and abs(lengths[0] - lengths[1]) > 0.3
    assert min(abs(float(np.dot(a, c))) / (np.linalg.norm(a) * np.linalg.norm(c)) for a, c in ((r, up), (r, f), (up, f))) > 0.03
    assert abs(r[1]) > 0.3 and abs(up[0]) > 0.2                             # rolled about the view axis
    sc, b, hit, nd, cont = parts("rolled_anamorphic_camera")              # [309 hits, 133 shadow rays, 176 continuations]
    assert hit.sum() >= 250 and (b["shadow"] == 1).sum() >= 100 and cont.sum() >= 150
    # the ring: every one of the seven instances is hit, three of them mirrored                                         [59 .. 159 hits each]
    sc, b, hit, nd, cont = parts("ring")
    neg, on = on_negative_det(sc, b, hit)
    assert len(sc.instances) == 7 and neg == [0, 2, 5] and np.bincount(b["inst"][hit], minlength=7).min() >= 50
    assert sorted(int(i["mesh"]) for i in sc.instances) == [0, 0, 0, 1, 1, 1, 1]


# ---- the fixtures can tell right from wrong -----------------------------------------------------------------------------------------------

NON_RIGID = [("sheared_mirrored_glass", 0), ("anisotropic_diffuse", 0), ("sheared_mirrored_glass_cube", 1), ("ring", 0), ("ring", 2), ("ring", 4), ("ring", 6)]


@pytest.mark.parametrize("key,inst", NON_RIGID)
def test_recorded_normals_reject_the_object_to_world_map(rig, key, inst):
    """A kernel that took the normal through the linear part L of object-to-world, normalize(L n), instead of n . w2o
    (src/shader.rchit:94: the inverse transpose) would be right on every rigid or uniformly scaled instance.  On these it is off by more
    than 1e-3 (a hundred times the replay bar) on at least half of the hits, while normalize(inverse(L)^T n) in binary64 is the record."""
    sc = rig.scenes[key]
    b = sc.bounces[sc.bounces["inst"] == inst]
    assert len(b) >= 50
    L = linear_parts(sc)[inst]
    n = object_normals(rig, sc, b)
    right = unit(n @ np.linalg.inv(L))           # row vector times w2o
    wrong = unit(n @ L.T)                        # L n
    assert np.abs(right - b["N"]).max() <= SPV_TOL
    off = np.abs(wrong - b["N"]).max(axis=1) > 1e-3
    assert off.mean() >= 0.5, (key, inst, float(off.mean()))


MIRRORED = [("sheared_mirrored_glass", 0), ("sheared_mirrored_glass_cube", 1), ("ring", 0), ("ring", 2), ("ring", 5)]


@pytest.mark.parametrize("key,inst", MIRRORED)
def test_recorded_branches_reject_a_flipped_normal(rig, key, inst):
    """On an instance with det < 0 a kernel that derived the normal's side from the triangle's winding, or flipped it with the sign of
    the determinant, would have -N.  The recorded branch — `outwards` of a glass hit, read from the side of the surface the next ray
    starts on; the back-face break of a diffuse hit — is the one N gives on every hit, and the one -N does not give on at least 99 % of
    them (all but the hits with |d . N| < 1e-3)."""
    sc = rig.scenes[key]
    b = sc.bounces
    b = b[b["inst"] == inst]
    typ = types_of(sc, b)[0]
    nd = dot(b["d"], b["N"])
    if typ == 2:
        b, nd = b[b["last"] == 0], nd[b["last"] == 0]
        off = np.asarray(b["no"], np.float64) - b["P"]                         # -+ 0.01 * (outwards ? -N : N)   (src/shader.rgen:158,164)
        reflected = dot(off, b["d"]) < 0                                       # total internal reflection starts on the incoming side
        recorded = np.where(reflected, dot(off, b["N"]) < 0, dot(off, b["N"]) > 0)
        branch = lambda x: x > 0.0                                             # bool outwards = ndoti > 0.0f
        assert reflected.sum() >= 20 and (~reflected).sum() >= 20
    else:
        assert typ == 0
        recorded = b["shadow"] == 0                                            # if (dot(rayDirection, hitNormal) >= 0) break;
        branch = lambda x: x >= 0.0
    # (both branches occur on the glass instances; a closed diffuse mesh seen from outside shows front faces only)
    assert len(b) >= 50 and (~recorded).any() and (recorded.any() or typ == 0)
    assert np.array_equal(branch(nd), recorded)
    assert (branch(-nd) != recorded).mean() >= 0.99 and (np.abs(nd) > 1e-3).mean() >= 0.99


# ---- replay, pixels, samples ---------------------------------------------------------------------------------------------------------------

def test_oracle_replays_the_edge_records(rig):
    """tests/spirv_replay.py on the edge set: primary rays, the oracle's own traversal bit for bit, bounce_step per record, at the base
    set's bars."""
    worst = replay_records(rig.scenes.values(), oracle_scene=rig.oracle_of)
    print("edge replay, worst absolute differences:", worst)
    assert set(worst) == {"primary ray", "sky colour", "payload.hitPosition", "payload.hitNormal", "shadow ray origin", "shadow ray direction",
                          "shadow ray tmax", "lit colour", "next rayOrigin", "next rayDirection"}
    for k, v in worst.items():
        assert v <= (SPV_TOL_LIT if k == "lit colour" else SPV_TOL), (k, v, worst)
    assert worst["sky colour"] == 0.0


@pytest.mark.parametrize("key", KEYS)
def test_oracle_pixels_match_the_edge_pixels(rig, key):
    """the bar of test_oracle_pixels_match_the_reference_spirv_pixels: 2e-4 on >= 99.5 % of the recorded pixels, alpha exactly 1"""
    sc = rig.select(key)
    px = sc.pixels
    img = rig.orc.render_pixels(sc.width, sc.height, np.stack([px["px"], px["py"]], axis=1))
    d = np.abs(img - px["rgba"]).max(axis=1)
    print("%s: pixels worst %.3g, within %g: %.4f" % (key, d.max(), PIXEL_TOL, (d <= PIXEL_TOL).mean()))
    assert (d <= PIXEL_TOL).mean() >= PIXEL_SHARE, (key, float((d <= PIXEL_TOL).mean()), float(d.max()))
    assert np.all(img[:, 3] == 1.0) and np.all(px["rgba"][:, 3] == 1.0)


def oracle_samples(rig, key):
    """the oracle's colour of every sample of every recorded pixel, from its OWN primary rays (tests/shade_reference.py), sample-major"""
    sc = rig.select(key)
    px, spp, W, H = sc.pixels, rig.spp(key), sc.width, sc.height
    od = np.array([rig.orc.primary_ray(int(p["px"]), int(p["py"]), W, H, i) for i in range(spp) for p in px])
    s = shade_samples(rig.orc, record_rays(od[:, 0:3], od[:, 3:6]), len(px), rig.max_bounce(key))
    # (the composed reference is the frame: its average is render_pixels bit for bit)
    ref = rig.orc.render_pixels(W, H, np.stack([px["px"], px["py"]], axis=1))
    assert np.array_equal(average_points(s, len(px), spp).view(np.uint32), ref.view(np.uint32))
    return s


@pytest.mark.parametrize("key", KEYS)
def test_oracle_samples_match_the_edge_samples(rig, key):
    """Per-sample colours: the oracle's colour of sample i of a recorded pixel (its own primary ray through tests/shade_reference.py)
    against tmpColor of that sample's last record.  Measured on this set, oracle against interpreter: the reference side meets the pixel
    bar on every scene, so it is the bar here too: >= 99.5 % of a scene's samples within 2e-4.  Worst absolute difference per scene
    (share within 2e-4 is 100 % where not given):
        sheared_mirrored_glass 2.35e-04 (99.86 %: one of 714 samples, a sky colour after five glass bounces)
        anisotropic_diffuse 4.95e-06   sheared_mirrored_glass_cube 6.08e-05   inside_glass 1.65e-04          inside_diffuse 0
        inside_mirror 1.19e-06         unknown_types 1.83e-05                 light_inside 0                 light_close 4.77e-07
        intensity_0 8.05e-07           intensity_3p5 1.83e-05                 depth0_spp1 8.05e-07           spp5 6.33e-07
        spp16 4.95e-06                 rolled_anamorphic_camera 4.02e-05      ring 1.79e-07
    The large ones are sky colours: a direction that differs in its last bits after several refractions moves the bilinear weights of a
    2048^2 cube face.  The lit colours, pow(0.9, float(i)) up to i = 15 included, are within 2e-5 (the replay test)."""
    _, last = rig.recorded_samples(key)
    s = oracle_samples(rig, key)
    d = np.abs(s[:, 0:3] - last["color"]).max(axis=1)
    print("%s: samples worst %.3g, within %g: %.4f" % (key, d.max(), PIXEL_TOL, (d <= PIXEL_TOL).mean()))
    assert (d <= PIXEL_TOL).mean() >= PIXEL_SHARE, (key, float((d <= PIXEL_TOL).mean()), float(d.max()))
    assert np.all(s[:, 3] == 1.0)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gpu(rig):
    """one context for the module: the meshes and the cube map go up once, a scene is its instances and uniforms"""
    from vulkan_raytracing_amd import RtContext
    c = RtContext(0)
    c.upload_geometry(rig.geom.verts, rig.geom.idx, rig.geom.ranges)
    c.set_skybox(rig.sky)

    def select(key):
        sc = rig.select(key)
        c.set_instances(sc.instances)
        c.set_uniforms(sc.uniforms)
        return sc
    c.select = select
    yield c
    c.close()


def counts(st):
    return (int(st.rays_primary), int(st.rays_secondary), int(st.rays_shadow))


def assert_pixel_bar(got, want, what):
    d = np.abs(np.asarray(got, np.float32) - want).max(axis=1)
    print("%s: worst %.3g, within %g: %.4f" % (what, d.max(), PIXEL_TOL, (d <= PIXEL_TOL).mean()))
    assert (d <= PIXEL_TOL).mean() >= PIXEL_SHARE, (what, float((d <= PIXEL_TOL).mean()), float(d.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_hip_frame_equals_the_oracle_and_meets_the_edge_pixels(rig, gpu, key):
    """G1: the frame is the oracle's bit for bit with identical ray counts — under the default launch parameters, with fused_shade 0 and
    pixel_beams 0 (one walk per ray, k_shade on its own), and with the instance records given in device memory (TLAS built on the GPU).
    G2: that frame against the recorded pixels at the bar of the CPU test."""
    import torch
    sc = gpu.select(key)
    W, H = sc.width, sc.height
    ref, rc = rig.oracle_frame(key)
    want = tuple(int(x) for x in rc)
    img, st = gpu.trace(W, H)
    assert_frame_equals_oracle(img, rig.orc, W, H, ref=ref)
    assert counts(st) == want
    try:
        gpu.set_param("fused_shade", 0); gpu.set_param("pixel_beams", 0)
        plain, st = gpu.trace(W, H)
        assert_frame_equals_oracle(plain, rig.orc, W, H, ref=ref)
        assert counts(st) == want
    finally:
        gpu.set_param("fused_shade", 1); gpu.set_param("pixel_beams", 1)
    t = torch.from_numpy(np.ascontiguousarray(sc.instances).view(np.uint8).reshape(-1, 64).copy()).to("cuda:0")
    torch.cuda.current_stream().synchronize()
    try:
        gpu.set_instances_device(t)
        dev, st = gpu.trace(W, H)
        assert_frame_equals_oracle(dev, rig.orc, W, H, ref=ref)
        assert counts(st) == want
    finally:
        gpu.set_instances(sc.instances)
    px = sc.pixels
    assert_pixel_bar(img[px["py"], px["px"]], px["rgba"], key + ": frame against the recorded pixels")
    assert np.all(img[..., 3] == 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_hip_ray_queries_match_the_edge_records(rig, gpu, key):
    """G3: the recorded closest-hit rays through rt_intersect_device with attributes — inst, prim, t, u, v are the records bit for bit,
    position and normal are the recorded payload within SPV_TOL, objectIndex is equal; the recorded shadow rays through the any-hit
    form — occlusion is the recorded isShadow."""
    import torch
    sc = gpu.select(key)
    b = sc.bounces
    q = gpu.intersect_device(torch.from_numpy(record_rays(b["o"], b["d"])).to("cuda:0"), attributes=True)
    torch.cuda.synchronize()
    h, attr = q.numpy()
    hit = b["inst"] >= 0
    assert np.array_equal(h["inst"], b["inst"]) and np.array_equal(h["prim"], b["prim"])
    for k in ("t", "u", "v"):
        assert np.array_equal(h[k][hit].view(np.uint32), b[k][hit].view(np.uint32)), (key, k)
    pos, nrm, obj = attr[:, 0:3].view(np.float32), attr[:, 4:7].view(np.float32), attr[:, 3]
    assert np.array_equal(obj, b["object_index"])
    if hit.any():
        dp, dn = np.abs(pos[hit] - b["P"][hit]).max(), np.abs(nrm[hit] - b["N"][hit]).max()
        print("%s: position worst %.3g, normal worst %.3g" % (key, dp, dn))
        assert dp <= SPV_TOL and dn <= SPV_TOL, (key, float(dp), float(dn))
    sh = b["shadow"] == 1
    if sh.any():
        srays = record_rays(b["so"][sh], b["sl"][sh], b["stmax"][sh])
        qa = gpu.intersect_device(torch.from_numpy(srays).to("cuda:0"), any_hit=True)
        torch.cuda.synchronize()
        assert np.array_equal(qa.numpy()[0]["inst"] >= 0, b["occluded"][sh] == 1), key


@pytest.mark.gpu
@pytest.mark.parametrize("key", KEYS)
def test_hip_shade_rays_match_the_edge_samples(rig, gpu, key):
    """G4: the recorded bounce-0 rays through rt_shade_rays_device, sample-major with n_samples = spp.  The per-sample colours are the
    oracle's for the same rays bit for bit and meet the per-sample bar against the records; the per-point colours meet the pixel bar
    against the recorded pixels."""
    import torch
    sc = gpu.select(key)
    first, last = rig.recorded_samples(key)
    spp, P = rig.spp(key), len(sc.pixels)
    want = rig.oracle_samples_of_recorded_rays(key)
    s, p = gpu.shade_rays_device(torch.from_numpy(record_rays(first["o"], first["d"])).to("cuda:0"), samples=spp)
    torch.cuda.synchronize()
    s, p = s.cpu().numpy(), p.cpu().numpy()
    bad = np.nonzero((s.view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, (key, len(bad), bad[:10], s[bad[:3]], want[bad[:3]])
    assert np.array_equal(p.view(np.uint32), average_points(want, P, spp).view(np.uint32))
    assert_pixel_bar(s[:, 0:3], last["color"], key + ": samples against the recorded samples")
    assert_pixel_bar(p, sc.pixels["rgba"], key + ": points against the recorded pixels")
    assert np.all(s[:, 3] == 1.0)
