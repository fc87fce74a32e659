"""CPU tests of the oracle (oracle/rt_oracle.cpp, oracle/ingest.py) against everything the reference
holds for this path: the OpConstant words of its precompiled shaders, its vendored OBJ loader's
output (golden), and the analytic known answers of SURVEY.md Appendix B."""
import hashlib
import json
import math
import os
import struct

import numpy as np
import pytest

from oracle import ingest, oracle
from tests import scenes
from vulkan_raytracing_amd import host

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def f32bits(x):
    return struct.unpack("<I", struct.pack("<f", float(np.float32(x))))[0]


def test_constants_match_reference_spirv():
    """Every float literal the oracle (and kernels.hip) uses is the one glslang baked into the
    reference's shaders/shader.rgen.spv."""
    spv = json.load(open(os.path.join(GOLD, "spv_constants.json")))
    bits = {int(b, 16) for b in spv["shader.rgen.spv"]["f32_bits"]}
    literals = [12.9898, 78.233, 1113.1, 43758.5453, 0.5, 2.0, 1.0, -1.0, 2.5, 0.001, 10000.0, 0.01, 0.2, 0.8, 100.0, 0.9, 1.52,
                0.08, 0.24]  # last two: Iamb*ka folded by glslang
    for lit in literals:
        assert f32bits(lit) in bits, lit
    # 1/ior: IEEE binary32 division gives the folded constant
    assert f32bits(np.float32(1.0) / np.float32(1.52)) in bits
    # shadow ray flags = Opaque|TerminateOnFirstHit|SkipClosestHit = 13, mask 0xFF, payload locations 0/1
    assert 13 in spv["shader.rgen.spv"]["u32"] and 255 in spv["shader.rgen.spv"]["u32"]
    # rchit: stride 6 floats per vertex, 3 indices per primitive
    assert 6 in spv["shader.rchit.spv"]["u32"] and 3 in spv["shader.rchit.spv"]["u32"]


def test_ingest_matches_reference_loader_golden(resources):
    g = json.load(open(os.path.join(GOLD, "ingest_golden.json")))["obj"]
    for name in ("cube", "cube_scene", "teapot"):
        o = ingest.parse_obj(os.path.join(resources, name + ".obj"))
        vidx, prims = ingest.flatten(o)
        nidx = np.asarray([i for s in o.shapes for i in s["nidx"]], np.int32)
        assert hashlib.sha256(o.vertices.tobytes()).hexdigest() == g[name]["vertices.f32"]["sha256"]
        assert hashlib.sha256(o.normals.tobytes()).hexdigest() == g[name]["normals.f32"]["sha256"]
        assert hashlib.sha256(vidx.tobytes()).hexdigest() == g[name]["vidx.u32"]["sha256"]
        assert hashlib.sha256(nidx.tobytes()).hexdigest() == g[name]["nidx.i32"]["sha256"]
        assert prims == g[name]["vidx.u32"]["count"] // 3
        assert [s["faces"] for s in o.shapes] == g[name]["faces.u32"]["head"][: len(o.shapes)]


def test_uniform_block_layout():
    u = ingest.pack_uniforms(prim_offset=2256, vert_offset=7212)
    assert len(u) == 104
    # offsets of SURVEY.md §8 a8
    assert struct.unpack_from("<3f", u, 0) == (0.0, 0.0, 20.0)
    assert struct.unpack_from("<3f", u, 48) == (0.0, 0.0, -1.0)
    assert struct.unpack_from("<3f", u, 64) == (5.0, 5.0, 5.0)
    assert struct.unpack_from("<f", u, 76) == (1.0,)
    assert struct.unpack_from("<6I", u, 80) == (63, 4, 1, 0, 2256, 7212)
    sa = ingest.SceneArrays([os.path.join(scenes.RES, "teapot.obj"), os.path.join(scenes.RES, "cube.obj")])
    assert sa.orbiting_primitive_offset == 2256 and sa.orbiting_vertex_offset == 1202 * 6  # main.cpp:1872-1873
    assert len(ingest.pack_instance(np.arange(12), 1)) == 64


def test_jitter_hash_canonical_values():
    L = oracle.lib()
    # SURVEY.md Appendix B samples, re-derived with the correctly rounded sine (numpy's float32 sin is
    # 1 ulp off at pixel (0,0) seed 4.0, which moves that sample from 0.234375 to 0.23046875)
    assert L.orc_jitter(0, 0, 4.0) == 0.23046875
    assert L.orc_jitter(0, 0, 4.5) == 0.203125
    assert (L.orc_jitter(1, 0, 4.0), L.orc_jitter(1, 0, 4.5)) == (0.296875, 0.9453125)
    assert (L.orc_jitter(1919, 1079, 4.0), L.orc_jitter(1919, 1079, 4.5)) == (0.921875, 0.359375)
    # definition check against an independent evaluation: float32 steps + libm double sin rounded once
    rng = np.random.default_rng(1)
    for _ in range(2000):
        px, py, seed = float(rng.integers(0, 3840)), float(rng.integers(0, 2160)), float(rng.integers(1, 17)) + (0.5 if rng.random() < 0.5 else 0.0)
        d = np.float32(np.float32(px) * np.float32(12.9898)) + np.float32(np.float32(py) * np.float32(78.233))
        a = np.float32(d + np.float32(np.float32(1113.1) * np.float32(seed)))
        s = np.float32(math.sin(float(a)))
        x = np.float32(s * np.float32(43758.5453))
        assert L.orc_jitter(px, py, seed) == float(x - np.floor(x))


def test_canonical_sine_accuracy():
    L = oracle.lib()
    rng = np.random.default_rng(0)
    xs = np.float32(rng.uniform(-4e5, 4e5, 20000))
    err = max(abs(L.orc_sin(float(x)) - math.sin(float(x))) for x in xs)
    assert err < 2.3e-16


def test_appendix_b_known_answers():
    """Independent float64 brute-force answers from SURVEY.md Appendix B."""
    sa = ingest.SceneArrays([os.path.join(scenes.RES, "teapot.obj")])
    S = oracle.OracleScene()
    S.set_geometry(sa.verts, sa.idx, sa.ranges)
    S.set_instances([ingest.pack_instance(ingest.glm_to_vulkan(ingest.mat_identity()), 0, mesh=0)])

    def ray(u, v):
        d = np.array([u, v, -2.5], np.float64)
        d /= np.linalg.norm(d)
        return [0, 0, 20, 0.001, d[0], d[1], d[2], 10000.0]

    for bvh in (False, True):
        h = S.intersect(np.array([ray(0.1, 0.1), ray(-0.12, 0.25), ray(0.5, 0.5)], np.float32), use_bvh=bvh)
        assert h["prim"][0] == 648 and abs(h["t"][0] - 18.211872) < 2e-5 and abs(h["u"][0] - 0.422183) < 2e-5 and abs(h["v"][0] - 0.164100) < 2e-5
        assert h["prim"][1] == 400 and abs(h["t"][1] - 18.595569) < 2e-5 and abs(h["u"][1] - 0.007822) < 2e-5 and abs(h["v"][1] - 0.884453) < 2e-5
        assert h["inst"][2] == -1
    a = S.hit_attributes(h)
    assert np.allclose(a[0, :6], [0.72731, 0.72731, 1.81720, 0.34838, -0.28454, 0.89313], atol=2e-5)
    assert np.allclose(a[1, :6], [-0.88715, 1.84822, 1.51779, -0.46033, 0.38678, 0.79906], atol=2e-5)
    # cube at T(0,0,5): z = 6 plane at t = 14.003248, N = (0,0,1)
    sa = ingest.SceneArrays([os.path.join(scenes.RES, "cube.obj")])
    S = oracle.OracleScene()
    S.set_geometry(sa.verts, sa.idx, sa.ranges)
    S.set_instances([ingest.pack_instance(ingest.glm_to_vulkan(ingest.mat_translate(ingest.mat_identity(), (0, 0, 5))), 1, mesh=0)])
    h = S.intersect(np.array([ray(0.05, 0.02), ray(0, 0)], np.float32))
    assert h["prim"][0] == 0 and abs(h["t"][0] - 14.003248) < 2e-5 and abs(h["u"][0] - 0.084) < 1e-5 and abs(h["v"][0] - 0.556) < 1e-5
    assert h["t"][1] == 14.0 and h["prim"][1] == 0  # tie on the shared edge resolved to the smaller primitive index
    a = S.hit_attributes(h)
    assert np.allclose(a[:, 2], 6.0) and np.allclose(a[:, 3:6], [0, 0, 1])


def test_bvh_equals_brute_force():
    """Property of SURVEY.md §4: BVH traversal == O(N) closest hit, any-hit == (closest t < tmax)."""
    sp = scenes.two_object_scene(os.path.join(scenes.RES, "teapot.obj"), os.path.join(scenes.RES, "cube.obj"), 1, 0, 1, 1)
    rays = scenes.random_rays(4000, seed=3)
    a = sp.orc.intersect(rays, use_bvh=True)
    b = sp.orc.intersect(rays, use_bvh=False)
    assert np.array_equal(a, b)
    assert (a["inst"] >= 0).mean() > 0.3
    sh = rays.copy(); sh[:, 7] = 18.0
    any_b = sp.orc.intersect(sh, any_hit=True, use_bvh=True)
    clo = sp.orc.intersect(sh, use_bvh=False)
    assert np.array_equal(any_b["inst"] >= 0, clo["inst"] >= 0)


def test_bvh_equals_brute_force_on_grazing_rays():
    """Rays that run almost parallel to a coordinate plane and skim box faces (what the rows through the image centre
    are: |d.y| ~ 1e-4 .. 1e-6).  One ulp of error in (plane - origin) is then 1e-3 .. 1e-1 in t, so a box test with slack
    on t alone culls triangles that lie on a box face — the axis-aligned faces of cube.obj lie on EVERY box face of its
    tree.  The oracle's BVH mode must still equal its brute-force mode (a whole-frame GPU comparison once differed from
    the BVH mode by one hit in 8.3 M and agreed with brute force)."""
    sp = scenes.two_object_scene(os.path.join(scenes.RES, "teapot.obj"), os.path.join(scenes.RES, "cube.obj"), 1, 0, 1, 1)
    rays = scenes.grazing_rays(60000, seed=11)
    a = sp.orc.intersect(rays, use_bvh=True)
    b = sp.orc.intersect(rays, use_bvh=False)
    assert (b["inst"] >= 0).mean() > 0.2
    assert np.array_equal(a, b), int((a != b).sum())


def test_refraction_and_tir_threshold():
    """TIR inside glass when sin(theta) > 1/1.52 (theta_c = 41.1395 deg), src/shader.rgen:139-165."""
    assert abs(math.degrees(math.asin(1 / 1.52)) - 41.1395) < 1e-3
    ratio = np.float32(1.52)
    for deg, tir in ((40.0, False), (42.0, True)):
        ndoti = -np.float32(math.cos(math.radians(deg)))
        k = np.float32(1.0) - (ratio * ratio) * (np.float32(1.0) - ndoti * ndoti)
        assert (k < 0) == tir


def test_cube_face_selection_and_flip():
    """Miss lookup direction is (d.x, d.y, -d.z) (src/shader.rgen:92); layers in the order of
    src/main.cpp:2064-2071.  Each face of the test cube map is a flat, distinct colour."""
    faces = []
    for f in range(6):
        img = np.zeros((8, 8, 4), np.uint8); img[..., 0] = 40 * f + 10; img[..., 1] = 255 - 40 * f; img[..., 3] = 255
        faces.append(img)
    S = oracle.OracleScene(); S.set_skybox(faces)
    for axis, layer in (((1, 0, 0), 0), ((-1, 0, 0), 1), ((0, 1, 0), 2), ((0, -1, 0), 3), ((0, 0, 1), 4), ((0, 0, -1), 5)):
        c = S.sample_sky(np.array(axis, np.float32))
        assert abs(c[0] * 255 - (40 * layer + 10)) < 1e-3
    # d = normalize(0.5,0.5,-2.5) -> lookup (.., .., +0.96) -> +Z = layer 4 = front.jpg
    d = np.array([0.5, 0.5, -2.5]); d /= np.linalg.norm(d)
    c = S.sample_sky(np.array([d[0], d[1], -d[2]], np.float32))
    assert abs(c[0] * 255 - (40 * 4 + 10)) < 1e-3


def test_bilinear_cube_filter_matches_float64():
    faces = scenes.synthetic_skybox(16, seed=5)
    S = oracle.OracleScene(); S.set_skybox(faces)
    rng = np.random.default_rng(2)
    for _ in range(500):
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        d[2] = abs(d[2]) + 1.5  # stay on +Z, away from the face edge
        d /= np.linalg.norm(d)
        c = S.sample_sky(d.astype(np.float32))
        s, t = 0.5 * (d[0] / d[2] + 1), 0.5 * (-d[1] / d[2] + 1)
        u, v = s * 16 - 0.5, t * 16 - 0.5
        x0, y0 = int(np.floor(u)), int(np.floor(v)); wu, wv = u - x0, v - y0
        f = faces[4].astype(np.float64)
        cl = lambda a: min(max(a, 0), 15)
        ref = ((f[cl(y0), cl(x0)] * (1 - wu) + f[cl(y0), cl(x0 + 1)] * wu) * (1 - wv) + (f[cl(y0 + 1), cl(x0)] * (1 - wu) + f[cl(y0 + 1), cl(x0 + 1)] * wu) * wv) / 255
        assert np.allclose(c, ref[:3], atol=2e-4)


def _smooth_cube(size):
    """cube map whose texels sample one smooth function of the direction (so that correct filtering is continuous everywhere)"""
    faces = []
    c = (np.arange(size) + 0.5) / size * 2.0 - 1.0
    s, t = np.meshgrid(c, c)
    one = np.ones_like(s)
    dirs = [(one, -t, -s), (-one, -t, s), (s, one, t), (s, -one, -t), (s, -t, one), (-s, -t, -one)]   # Appendix C, inverted
    for (x, y, z) in dirs:
        n = np.sqrt(x * x + y * y + z * z)
        x, y, z = x / n, y / n, z / n
        img = np.zeros((size, size, 4), np.uint8)
        img[..., 0] = np.round(127.5 + 127.5 * np.sin(3.0 * x + 1.0) * np.cos(2.0 * y - 0.5))
        img[..., 1] = np.round(127.5 + 127.5 * np.sin(2.5 * z + 0.3) * np.cos(3.0 * x + y))
        img[..., 2] = np.round(127.5 + 127.5 * np.sin(4.0 * y + 2.0 * z))
        img[..., 3] = 255
        faces.append(img)
    return faces


def _edge_directions(n_along, eps):
    """pairs of directions straddling each of the 12 cube edges (and, with |w| -> 1, approaching the 8 corners)"""
    pairs = []
    for a in range(3):                       # the two axes that are tied along an edge: (a, b); the third runs along it
        for b in range(a + 1, 3):
            c = 3 - a - b
            for sa in (-1.0, 1.0):
                for sb in (-1.0, 1.0):
                    for w in np.linspace(-0.97, 0.97, n_along):
                        lo, hi = np.zeros(3), np.zeros(3)
                        lo[a], lo[b], lo[c] = sa * (1.0 + eps), sb * 1.0, w      # |a| major
                        hi[a], hi[b], hi[c] = sa * 1.0, sb * (1.0 + eps), w      # |b| major
                        pairs.append((lo, hi))
    return pairs


def test_cube_filtering_is_seamless_across_all_twelve_edges():
    """VK_FILTER_LINEAR on a cube view takes footprint texels that fall off the selected face from the neighbouring face
    (src/main.cpp:2393-2406; Vulkan 'cube map edge handling'): the filtered colour is continuous across every edge.  A
    per-face clamp (round 1) jumps there by up to half a texel's gradient (~0.05 on this 16^2 map)."""
    S = oracle.OracleScene()
    S.set_skybox(_smooth_cube(16))
    worst = 0.0
    for lo, hi in _edge_directions(25, 1e-5):
        worst = max(worst, float(np.abs(S.sample_sky(lo.astype(np.float32)) - S.sample_sky(hi.astype(np.float32))).max()))
    assert worst < 2e-3, worst


def test_cube_edge_and_corner_taps_match_an_independent_float64_sampler():
    """Directions within half a texel of every edge and corner against a float64 sampler written differently: every tap is
    located by projecting its texel CENTRE (on the extended face plane) back onto the cube and taking the nearest texel
    there; the tap beyond a corner is the mean of the other three."""
    size = 8
    faces = _smooth_cube(size)
    rng = np.random.default_rng(5)
    for f in faces:
        f[..., :3] = rng.integers(0, 256, f[..., :3].shape)      # uncorrelated texels: a wrong neighbour cannot hide
    S = oracle.OracleScene()
    S.set_skybox(faces)
    tex = np.stack(faces).astype(np.float64)[..., :3]

    def face_of(r):
        ax = np.abs(r)
        if ax[2] >= ax[0] and ax[2] >= ax[1]:
            return (4, r[0], -r[1], ax[2]) if r[2] >= 0 else (5, -r[0], -r[1], ax[2])
        if ax[1] >= ax[0]:
            return (2, r[0], r[2], ax[1]) if r[1] >= 0 else (3, r[0], -r[2], ax[1])
        return (0, -r[2], -r[1], ax[0]) if r[0] >= 0 else (1, r[2], -r[1], ax[0])

    def point_on(layer, s, t):
        return np.array({0: (1, -t, -s), 1: (-1, -t, s), 2: (s, 1, t), 3: (s, -1, -t), 4: (s, -t, 1), 5: (-s, -t, -1)}[layer], np.float64)

    def ref(r):
        layer, sc, tc, ma = face_of(np.asarray(r, np.float64))
        u, v = 0.5 * (sc / ma + 1.0) * size - 0.5, 0.5 * (tc / ma + 1.0) * size - 0.5
        x0, y0 = int(np.floor(u)), int(np.floor(v))
        wu, wv = u - x0, v - y0
        taps, missing = {}, None
        for k, (x, y) in enumerate(((x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1))):
            ox, oy = not (0 <= x < size), not (0 <= y < size)
            if ox and oy:
                missing = k
                continue
            if ox or oy:
                l2, s2, t2, m2 = face_of(point_on(layer, (2 * x + 1) / size - 1.0, (2 * y + 1) / size - 1.0))
                xx = min(size - 1, int(np.floor(0.5 * (s2 / m2 + 1.0) * size)))
                yy = min(size - 1, int(np.floor(0.5 * (t2 / m2 + 1.0) * size)))
                taps[k] = tex[l2, yy, xx]
            else:
                taps[k] = tex[layer, y, x]
        if missing is not None:
            taps[missing] = sum(taps.values()) / 3.0
        a = taps[0] * (1 - wu) + taps[1] * wu
        b = taps[2] * (1 - wu) + taps[3] * wu
        return (a * (1 - wv) + b * wv) / 255.0

    n_corner = 0
    dirs = [p for pair in _edge_directions(9, 0.4 / size) for p in pair]
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                for _ in range(12):
                    dirs.append(np.array([sx, sy, sz], np.float64) * (1.0 - rng.uniform(0, 0.9 / size, 3)))
    for r in dirs:
        got = S.sample_sky(np.asarray(r, np.float32))
        want = ref(np.asarray(r, np.float32).astype(np.float64))
        assert np.abs(got - want).max() < 2e-6, (r, got, want)
        layer, sc, tc, ma = face_of(np.asarray(r, np.float64))
        u, v = 0.5 * (sc / ma + 1.0) * size - 0.5, 0.5 * (tc / ma + 1.0) * size - 0.5
        n_corner += (u < 0 or u > size - 1) and (v < 0 or v > size - 1)
    assert n_corner >= 40       # footprints that straddle three faces were exercised


def test_invert_affine_and_pow100():
    L = oracle.lib()
    rng = np.random.default_rng(4)
    for _ in range(50):
        m = np.zeros(12, np.float32); m[:] = rng.normal(size=12)
        out = np.zeros(12, np.float32)
        L.orc_invert_affine(m.ctypes.data, out.ctypes.data)
        A = np.vstack([m.reshape(3, 4).astype(np.float64), [0, 0, 0, 1]]); B = np.vstack([out.reshape(3, 4).astype(np.float64), [0, 0, 0, 1]])
        assert np.allclose(A @ B, np.eye(4), atol=1e-4 * max(1, np.abs(B).max()))
    for x in (0.0, 0.5, 0.97, 0.999, 1.0):
        assert abs(L.orc_pow100(x) - x ** 100) <= 2e-5 * max(x ** 100, 1e-30) + 1e-38


def test_cfg1_cube_scene_render_and_shading_terms():
    """BASELINE config 1: cube_scene.obj, 256x256, depth 1 (maxBounceCount 0), spp 1, CPU only.
    Checked against an independent numpy evaluation of the shading formula at a few pixels."""
    path = os.path.join(scenes.RES, "cube_scene.obj")
    inst = [ingest.pack_instance(ingest.glm_to_vulkan(ingest.mat_identity()), 0, mesh=0)]
    u = np.frombuffer(ingest.pack_uniforms(max_bounce=0, spp=1, center_type=0, orbit_type=0), dtype=np.uint8)
    sa = ingest.SceneArrays([path])
    S = oracle.OracleScene(); S.set_geometry(sa.verts, sa.idx, sa.ranges)
    S.set_instances(inst); S.set_uniforms(u.tobytes()); S.set_skybox(scenes.synthetic_skybox(32))
    img, rc = S.render(256, 256, threads=4)
    img2, _ = S.render(256, 256, threads=1, use_bvh=False)
    assert np.array_equal(img, img2)                     # BVH == brute force, threads irrelevant
    assert rc[0] == 256 * 256 and rc[1] == 0             # primary only
    assert np.all(img[..., 3] == 1.0)
    hit = np.any(np.abs(img[..., :3] - np.float32([0.08, 0.24, 0.08])) > 0, axis=2)
    # every pixel is sky, ambient, or ambient + lit term (green-dominant because kd = (0.2,1,0.2))
    checked = 0
    for py in range(8, 256, 16):
        for px_ in range(8, 256, 16):
            o6 = S.primary_ray(px_, py, 256, 256, 0)
            rays = np.array([[o6[0], o6[1], o6[2], 0.001, o6[3], o6[4], o6[5], 10000.0]], np.float32)
            h = S.intersect(rays)
            if h["inst"][0] < 0:
                continue
            a = S.hit_attributes(h)[0].astype(np.float64)
            P, N, d = a[0:3], a[3:6], o6[3:6].astype(np.float64)
            exp = np.array([0.08, 0.24, 0.08])
            if np.dot(d, N) < -1e-4:
                Lv = np.array([5, 5, 5.0]) - P; dist = np.linalg.norm(Lv); Lv /= dist
                sh = S.intersect(np.array([[*(P + 0.01 * N), 0.001, *Lv, dist]], np.float32), any_hit=True)
                if sh["inst"][0] < 0:
                    Hh = Lv - d; Hh /= np.linalg.norm(Hh)
                    exp = exp + np.array([0.2, 1.0, 0.2]) * max(0, N @ Lv) + 0.8 * max(0, N @ Hh) ** 100
            elif np.dot(d, N) < 1e-4:
                continue
            assert np.allclose(img[py, px_, :3], exp, atol=5e-5), (px_, py)
            checked += 1
    assert checked >= 10 and hit.any()


def test_oracle_frames_match_their_committed_hashes():
    """The oracle's own regression goldens (tests/golden/oracle_images.json, written by make_oracle_images.py):
    bit-identical frames and ray counts.  They pin the oracle to its own past, not to the reference."""
    import importlib.util
    import json
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_oracle_images", os.path.join(here, "make_oracle_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = json.load(open(os.path.join(here, "oracle_images.json")))
    got = {name: mod.render_record(sp, W, H) for name, (sp, W, H) in mod.cases().items()}
    assert set(got) == set(want)
    for name in want:
        assert got[name]["rays"] == want[name]["rays"], name
        assert got[name]["sha256"] == want[name]["sha256"], name


def test_native_build_of_the_oracle_is_bit_identical():
    """bench.py's cpu_baseline times the oracle built -O3 -march=native (oracle/Makefile librt_oracle_native.so, compiled on the
    machine that runs it).  Same source, same -ffp-contract=off: the frames must equal the committed hashes of the portable
    build bit for bit — the canonical arithmetic does not depend on optimisation level or instruction set."""
    import hashlib
    import importlib.util
    import json
    from oracle import oracle
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_oracle_images", os.path.join(here, "make_oracle_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = json.load(open(os.path.join(here, "oracle_images.json")))
    for name, (sp, W, H) in mod.cases().items():
        S = oracle.OracleScene(native=True)
        S.set_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        S.set_instances([sp.instances[i].tobytes() for i in range(len(sp.instances))])
        S.set_uniforms(sp.uniforms.tobytes())
        S.set_skybox(sp.sky)
        img, rc = S.render(W, H)
        assert hashlib.sha256(np.ascontiguousarray(img, np.float32).tobytes()).hexdigest() == want[name]["sha256"], name
        assert [int(x) for x in rc] == want[name]["rays"], name


def test_division_free_over_255_equals_ieee_division(tmp_path):
    """kernels.hip computes x/255 in the cube-map filter with two fmas instead of an IEEE division; the oracle divides.
    tools/check_div255.c proves both agree for every binary32 x in [0, 256] (exhaustive with stride 1); here every
    61st value is checked so that the CPU suite stays fast."""
    import subprocess
    exe = str(tmp_path / "check_div255")
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "check_div255.c")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-o", exe, src, "-lm", "-lpthread"], check=True)
    r = subprocess.run([exe, "61"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mismatches 0" in r.stdout, r.stdout


# ---- the reference's own compiled shaders as the judge of the restatement ---------------------------------------------------
# tests/golden/spirv_fixtures.npz was produced by INTERPRETING /root/reference/shaders/*.spv (make_spirv_fixtures.py; the binaries
# are read as data, the traversal / inverse transform / cube sampler are bound to the oracle).  Every record is one iteration
# of the bounce loop as the reference's binaries executed it.  Bars: 1e-5 absolute (GLSL leaves the precision of normalize /
# reflect / pow / dot open, so bit equality with any one implementation is not defined), 2e-5 on the lit colour because
# pow(x, 100) by repeated squaring carries up to ~100 half-ulps of a term <= 0.8.  The replay loop is tests/spirv_replay.py, shared
# with the edge set of tests/test_spirv_edge.py.
from tests.spirv_replay import SPV_TOL, SPV_TOL_LIT, replay_records  # noqa: E402


@pytest.fixture(scope="module")
def spirv_fixture_scenes():
    return scenes.load_spirv_fixtures()


def test_spirv_fixture_covers_every_branch_of_the_shaders(spirv_fixture_scenes):
    b = np.concatenate([sc.bounces for sc in spirv_fixture_scenes])
    p = np.concatenate([sc.pixels for sc in spirv_fixture_scenes])
    assert len(b) > 10000 and len(p) > 3000 and len(spirv_fixture_scenes) == 7
    miss, hit = b["inst"] < 0, b["inst"] >= 0
    assert miss.sum() > 1000 and hit.sum() > 5000
    assert (b["shadow"] == 1).sum() > 2000 and ((b["shadow"] == 1) & (b["occluded"] == 0)).sum() > 500 and ((b["shadow"] == 1) & (b["occluded"] == 1)).sum() > 500
    assert (b["last"] == 0).sum() > 2000                       # mirror / refract / TIR continuations
    assert (hit & (b["shadow"] == 0) & (b["last"] == 1)).sum() > 10   # back-face break or bounce budget exhausted
    assert b["bounce"].max() >= 5 and b["sample"].max() == 3
    assert set(np.unique(b["object_index"])) == {-1, 0, 1}


def test_oracle_replays_the_reference_spirv_records(spirv_fixture_scenes):
    """rgen prologue (jitter hash, primary ray), rchit (closest_hit_attributes) and one bounce-loop iteration (bounce_step)
    against what the reference's shader.rgen.spv / shader.rchit.spv / miss modules computed for the same inputs."""
    worst = replay_records(spirv_fixture_scenes)
    for k, v in worst.items():
        assert v <= (SPV_TOL_LIT if k == "lit colour" else SPV_TOL), (k, v, worst)
    assert worst["sky colour"] == 0.0 and worst["primary ray"] <= 2.5e-7


def test_oracle_pixels_match_the_reference_spirv_pixels(spirv_fixture_scenes):
    """Whole pixels (sample loop, accumulation, division; src/shader.rgen:64-70,180-185) against the values the interpreted
    shader.rgen.spv wrote with OpImageWrite.  The oracle traces its OWN rays here, which differ from the recorded ones in the
    last bit (normalize, fma): a ray may then fall on the other side of a triangle edge, and a 1-ulp change of a sky direction
    moves the bilinear weights of a 2048^2 JPEG face by 1e-4 texel — hence 2e-4 and an outlier budget of 0.5 %."""
    for sc in spirv_fixture_scenes:
        S, px = sc.oracle_scene(), sc.pixels
        img = S.render_pixels(sc.width, sc.height, np.stack([px["px"], px["py"]], axis=1))
        d = np.abs(img - px["rgba"]).max(axis=1)
        assert (d <= 2e-4).mean() >= 0.995, (sc.name, float((d <= 2e-4).mean()), float(d.max()))
        assert np.all(img[:, 3] == 1.0) and np.all(px["rgba"][:, 3] == 1.0)


# ---- MTL materials and a per-instance type table ------------------------------------------------------
def test_integer_power_matches_pow100_and_small_cases():
    L = oracle.lib()
    rng = np.random.default_rng(2)
    xs = np.concatenate([rng.uniform(0, 1, 4000), [0.0, 1.0, 0.5, 1.0 - 1e-6, 1e-3]]).astype(np.float32)
    for x in xs:
        assert np.float32(L.orc_pow_int(float(x), 100)).view(np.uint32) == np.float32(L.orc_pow100(float(x))).view(np.uint32)
    x = np.float32(0.83)
    assert L.orc_pow_int(float(x), 0) == 1.0 and np.float32(L.orc_pow_int(float(x), 1)) == x
    assert np.float32(L.orc_pow_int(float(x), 3)) == np.float32(np.float32(x * x) * x)          # x^2 * x^1, highest bit first
    assert abs(L.orc_pow_int(float(x), 225) - float(x) ** 225) < 1e-6 * float(x) ** 225 * 300


def test_materials_drive_the_diffuse_and_refractive_branches():
    """With a material table the diffuse branch uses the hit triangle's Ka/Kd/Ks/Ns and the refractive branch its Ni; the
    lit colour is checked against the Blinn-Phong formula of src/shader.rgen:116-128 evaluated in float64; an `illum`-derived
    material type overrides the instance's; without the table nothing changes."""
    from vulkan_raytracing_amd.api import MATERIAL_DTYPE, MATERIAL_TYPE_OF_INSTANCE
    from oracle.oracle import HIT_DTYPE
    inst = [host.make_instance(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), 0, 0)]
    u = host.default_uniforms(max_bounce_count=2, samples_per_pixel=1, center_object_type=0, orbiting_object_type=0)
    sp = scenes.ScenePair([os.path.join(scenes.RES, "cube_scene.obj")], inst, u, sky=scenes.synthetic_skybox(32))
    g = sp.geom
    assert len(g.materials) == 9 and len(g.prim_material) == g.ranges[0][2] and set(np.unique(g.prim_material)) == set(range(1, 9))
    assert np.allclose(g.materials[0]["kd"], [0.2, 1.0, 0.2]) and g.materials[0]["ns"] == 100.0 and g.materials[0]["type"] == MATERIAL_TYPE_OF_INSTANCE
    W = H = 64
    base, _ = sp.orc.render(W, H)
    sp.set_materials(g.materials, g.prim_material)
    with_mtl, _ = sp.orc.render(W, H)
    assert np.abs(with_mtl - base).max() > 0.05                 # the MTL colours differ from the hard-coded green
    # lit samples against the formula
    xy = np.array([(x, y) for y in range(8, 56, 3) for x in range(8, 56, 3)], np.uint32)
    rays = np.zeros((len(xy), 8), np.float32)
    for k, (x, y) in enumerate(xy):
        od = sp.orc.primary_ray(int(x), int(y), W, H, 0)
        rays[k] = (od[0], od[1], od[2], 0.001, od[3], od[4], od[5], 10000.0)
    h = sp.orc.intersect(rays)
    hits = h[h["inst"] >= 0]
    r = rays[h["inst"] >= 0]
    st = sp.orc.bounce_step(np.concatenate([r[:, 0:3], r[:, 4:7]], axis=1), np.zeros(len(r), np.uint32), hits)
    shadow = st[:, 0] == 2
    assert shadow.sum() > 50
    light = np.array([5.0, 5.0, 5.0])
    checked = 0
    for k in np.nonzero(shadow)[0]:
        m = g.materials[g.prim_material[hits[k]["prim"]]]
        P, N, d = st[k, 1:4].astype(np.float64), st[k, 4:7].astype(np.float64), r[k, 4:7].astype(np.float64)
        Lv = (light - P) / np.linalg.norm(light - P)
        Hh = (Lv - d) / np.linalg.norm(Lv - d)
        want = 0.8 * m["ka"].astype(np.float64) + m["kd"] * max(0.0, N @ Lv) + m["ks"] * max(0.0, N @ Hh) ** round(float(m["ns"]))
        assert np.abs(st[k, 15:18] - want).max() < 2e-5, (k, st[k, 15:18], want)
        checked += 1
    assert checked > 50
    # an `illum 3` material turns its faces into mirrors whatever the instance says; Ni feeds the refraction ratio
    tbl = g.materials.copy()
    tbl["type"][1:] = 1
    sp.set_materials(tbl, g.prim_material)
    assert np.all(sp.orc.bounce_step(np.concatenate([r[:, 0:3], r[:, 4:7]], axis=1), np.zeros(len(r), np.uint32), hits)[:, 0] == 3)
    tbl["type"][1:] = 2
    tbl["ni"][1:] = 1.0                                          # index 1: the ray goes straight on
    sp.set_materials(tbl, g.prim_material)
    st2 = sp.orc.bounce_step(np.concatenate([r[:, 0:3], r[:, 4:7]], axis=1), np.zeros(len(r), np.uint32), hits)
    assert np.all(st2[:, 0] == 3) and np.abs(st2[:, 21:24] - r[:, 4:7]).max() < 1e-6
    sp.set_materials(None)
    again, _ = sp.orc.render(W, H)
    assert np.array_equal(again, base)
    # the reference's own surface as an explicit table: the same image up to the one rounding of 0.8f * 0.1f vs the folded 0.08f
    ref_tbl = g.materials[:1].copy()
    sp.set_materials(ref_tbl, np.zeros(len(g.prim_material), np.uint32))
    assert np.abs(sp.orc.render(W, H)[0] - base).max() < 1e-6


def test_per_instance_types_replace_the_two_way_switch():
    """src/shader.rgen:96 maps objectIndex 0 / non-0 to two uniform fields; rt_set_instance_types gives every instance its
    own type (here three instances of the cube: diffuse, mirror, refractive)."""
    cube = os.path.join(scenes.RES, "cube.obj")
    inst = np.zeros(3, scenes.INSTANCE_DTYPE)
    for k, x in enumerate((-3.0, 0.0, 3.0)):
        inst[k] = host.make_instance(np.array([1, 0, 0, x, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), 1, 0)
    u = host.default_uniforms(max_bounce_count=3, samples_per_pixel=1, center_object_type=1, orbiting_object_type=0)
    sp = scenes.ScenePair([cube], inst, u, sky=scenes.synthetic_skybox(32))
    rays = np.array([[x, 0.2, 20, 0.001, 0, 0, -1, 10000.0] for x in (-3.0, 0.1, 3.0)], np.float32)
    h = sp.orc.intersect(rays)
    assert list(h["inst"]) == [0, 1, 2]
    od = np.concatenate([rays[:, 0:3], rays[:, 4:7]], axis=1)
    assert list(sp.orc.bounce_step(od, np.zeros(3, np.uint32), h)[:, 0]) == [2, 2, 2]       # customIndex 1 everywhere: all diffuse
    sp.set_instance_types([0, 1, 2])
    st = sp.orc.bounce_step(od, np.zeros(3, np.uint32), h)
    assert list(st[:, 0]) == [2, 3, 3]
    assert np.allclose(st[1, 21:24], [0, 0, 1], atol=1e-6)                                  # mirror: straight back
    assert np.allclose(st[2, 21:24], [0, 0, -1], atol=1e-6) and st[2, 20] < 1.0             # glass, normal incidence: straight on, origin pushed inside
    sp.set_instance_types(None)
    assert list(sp.orc.bounce_step(od, np.zeros(3, np.uint32), h)[:, 0]) == [2, 2, 2]
