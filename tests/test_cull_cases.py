"""The inputs of tests/test_cull_fuzz.py, checked without a GPU (tests/cull_cases.py): every case is what its family says (predicates in
binary64 over the binary32 records and uniforms), every family has enough cases, the cases are not empty frames, and the oracle can
referee them — its frame is finite and its tree mode equals its brute-force mode bit for bit, ray counts included."""
import numpy as np
import pytest

from tests import closest_reference, cull_cases as cc, scenes
from vulkan_raytracing_amd import host

SEED = cc.DEFAULT_SEED
MIN_CASES = 8
# families whose frames may be empty of something by construction (everything else has to show hits, shadow rays and secondary rays)
MAY_LACK_SHADOW_RAYS = {"near_singular": "the rays of a nearly singular basis fan out in one plane: a third of them is not promised diffuse hits"}


@pytest.fixture(scope="module")
def cases():
    """[(scene, pose, geometry, frame, ray counts, brute-force frame, brute-force ray counts, primary hit pixels)] of the default seed;
    the oracle renders every case twice (tree and brute force) and once with every instance masked (the sky alone)"""
    out, refused = [], []
    for sc in cc.scenes(SEED):
        sp = scenes.ScenePair(sc.paths, sc.instances, sc.uniforms, sky=sc.sky)
        sp.set_instance_types(sc.types)
        frames = {}

        def accept(p):
            sp.set_instances(p.instances); sp.set_uniforms(p.uniforms)
            frames[p.name] = sp.orc.render(p.W, p.H)
            ok = bool(np.isfinite(frames[p.name][0]).all())
            if not ok:
                refused.append(p.name)
            return ok

        for p in list(cc.poses(sc, SEED, accept=accept)):
            if p.name not in frames:      # (the quoted close-up is not drawn: it is not replaced either)
                accept(p)
            sp.set_instances(p.instances); sp.set_uniforms(p.uniforms)
            img, rc = frames[p.name]
            bf, rc_bf = sp.orc.render(p.W, p.H, use_bvh=False)
            hidden = p.instances.copy()
            hidden["custom_index_and_mask"] &= 0x00FFFFFF
            sp.set_instances(hidden)
            sky, _ = sp.orc.render(p.W, p.H)
            out.append((sc, p, sp.geom, img, rc, bf, rc_bf, int((img.view(np.uint32) != sky.view(np.uint32)).any(axis=2).sum())))
    return out, refused


def test_generated_meshes_have_the_boxes_the_generator_places_against():
    geom = host.SceneGeometry(cc.mesh_paths())
    v = np.asarray(geom.verts, np.float64)
    assert [pc for _, _, pc in geom.ranges] == [12, 2256, 2, 2, 8]
    for m, (ff, fi, pc) in enumerate(geom.ranges):
        ix = np.asarray(geom.idx[fi:fi + 3 * pc], np.int64)
        p = v[ff:].reshape(-1, 6)[ix, :3]
        assert np.allclose(p.min(0), cc.MESH_LO[m], atol=1e-5) and np.allclose(p.max(0), cc.MESH_HI[m], atol=1e-5), cc.MESHES[m]
    sliver = cc.MESH_HI[cc.SLIVER] - cc.MESH_LO[cc.SLIVER]
    assert sliver[2] / sliver[0] == pytest.approx(1e-3)


def test_scenes_are_what_the_generator_promises():
    n = 0
    for sc in cc.scenes(SEED):
        n += 1
        masks = sc.instances["custom_index_and_mask"] >> 24
        assert 1 <= len(sc.instances) <= 6 and (masks == 0).sum() == 1
        seen = set(sc.types[:len(sc.instances)][masks != 0].tolist())
        assert {1, 2} <= seen, sc.name
        assert sc.mesh_of[cc.FLOOR_I] == cc.FLOOR and sc.types[cc.FLOOR_I] == 0
        assert int(sc.uniforms[0]["max_bounce_count"]) in (0, 1, 2, 3) and int(sc.uniforms[0]["samples_per_pixel"]) in (1, 2, 4, 5)
        for r in sc.instances:
            s = np.linalg.svd(cc.matrix(r)[:, :3], compute_uv=False)
            assert 0.04 <= s.min() and s.max() <= 30.0, (sc.name, s)      # scales 0.05 .. 20 (shear stretches the singular values a little)
    assert n == cc.N_SCENES
    a = [p.uniforms.tobytes() + p.instances.tobytes() for sc in cc.scenes(SEED) for p in cc.poses(sc, SEED)]
    b = [p.uniforms.tobytes() + p.instances.tobytes() for sc in cc.scenes(SEED) for p in cc.poses(sc, SEED)]
    assert a == b and len(set(a)) == len(a)       # seeded: the same cases every time, no two alike


def _corners(pose, k):
    M = cc.matrix(pose.instances[k]); mesh = int(pose.instances[k]["mesh"])
    c = np.array([[(cc.MESH_HI if (j >> a) & 1 else cc.MESH_LO)[mesh][a] for a in range(3)] for j in range(8)])
    return c @ M[:, :3].T + M[:, 3]


def _in_box(pose, k, p):
    w = _corners(pose, k)
    return bool(np.all(p >= w.min(0)) and np.all(p <= w.max(0)))


def _nearest(pose, geom, p):
    ref = closest_reference.Scene(geom.verts, geom.idx, geom.ranges, pose.instances)
    return float(closest_reference.brute64(ref, np.concatenate([p, [0.0]])[None])["t"][0])


def _check_camera(sc, pose, geom):
    fam, m = pose.families[0], pose.meta["camera"]
    pos = pose.vec("position")
    r, u, f = pose.vec("right"), pose.vec("up"), pose.vec("forward")
    det = np.linalg.det(np.stack([r, u, f], axis=1))
    if fam != "near_singular":
        assert cc.camera_det_ratio(pose) > 1e3
    if fam in ("shell", "in_box", "in_mesh", "wide", "long_lens", "subpixel_on_tile_corner", "far_origin_closeup"):
        assert det < 0                                            # the handedness of the reference's camera: right x up = -forward
    if fam == "in_box":
        k = m["inst"]
        assert _in_box(pose, k, pos) and not cc.inside_mesh(pose.instances[k], int(pose.instances[k]["mesh"]), pos)
    elif fam == "in_mesh":
        k = m["inst"]
        assert int(pose.instances[k]["mesh"]) in (cc.CUBE, cc.OCTA) and cc.inside_mesh(pose.instances[k], int(pose.instances[k]["mesh"]), pos)
    elif fam == "on_box_plane":
        w = _corners(pose, m["inst"])
        assert pos[m["axis"]] == m["plane"] and m["plane"] in (w[:, m["axis"]].min(), w[:, m["axis"]].max())
        assert np.count_nonzero(np.abs(f) > 0) == 1
        depth = (w - pos) @ f
        if abs(f[m["axis"]]) == 1.0:
            assert (depth == 0.0).sum() == 4                      # four corners at depth exactly 0
    elif fam == "axis_view":
        for v in (r, u, f):
            assert sorted(np.abs(v).tolist()) == [0.0, 0.0, 1.0]
    elif fam == "grazing":
        ang = np.arcsin(abs(np.dot(f, m["normal"])) / np.linalg.norm(f))
        assert 1e-4 * 0.9 <= ang <= 1e-2 * 1.1 and ang == pytest.approx(m["angle"], rel=0.1)
    elif fam in ("wide", "long_lens"):
        assert np.linalg.norm(f) == pytest.approx(m["forward_scale"], rel=1e-5)
        assert abs(np.linalg.norm(r) - np.linalg.norm(u)) > 0.15
    elif fam == "left_handed":
        assert det > 0                                            # mirrored against the reference's camera (whose det is -1)
    elif fam == "near_singular":
        assert cc.camera_det_ratio(pose) == pytest.approx(m["ratio"], rel=0.05) and m["ratio"] in (0.5, 2.0)
        assert np.linalg.norm(np.cross(r, u)) / (np.linalg.norm(r) * np.linalg.norm(u)) < 1e-4
    elif fam == "subpixel_on_tile_corner":
        k = m["inst"]
        px, py, az = cc.project(pose, cc.matrix(pose.instances[k])[:, 3])
        assert az > 0 and abs(px - m["pixel"][0]) < 0.05 and abs(py - m["pixel"][1]) < 0.05      # (the record's translation is binary32)
        on_corner = m["pixel"][0] in (0, pose.W) and m["pixel"][1] in (0, pose.H)
        assert on_corner or (m["pixel"][0] % 8 == 0 and m["pixel"][1] % 8 == 0 and 0 < m["pixel"][0] < pose.W and 0 < m["pixel"][1] < pose.H)
        s = np.linalg.svd(cc.matrix(pose.instances[k])[:, :3], compute_uv=False)
        assert 0.001 * 0.99 <= s.min() and s.max() <= 0.01 * 1.01
        q = np.array([cc.project(pose, c)[:2] for c in _corners(pose, k)])
        assert (q.max(0) - q.min(0)).max() < 2.0                  # the whole object within two pixels
    elif fam == "off_screen_edge":
        q = np.array([cc.project(pose, c) for c in _corners(pose, m["inst"])])
        if m["kind"] == "camera_plane":
            assert (q[:, 2] > 0).any() and (q[:, 2] < 0).any()    # corners on both sides of the camera plane
        else:
            front = q[q[:, 2] > 0]
            inside = (front[:, 0] > 0) & (front[:, 0] < pose.W) & (front[:, 1] > 0) & (front[:, 1] < pose.H)
            assert inside.any() and (not inside.all() or len(front) < 8)
    elif fam == "far_origin_closeup":
        k = m["inst"]
        assert np.abs(m["shift"]).min() >= 300.0 and np.abs(pos - m["shift"]).max() < 40.0 or m.get("quoted")
        d = np.linalg.norm(cc.matrix(pose.instances[k])[:, 3] - pos)
        assert 0.003 * 0.5 <= d <= 0.02 * 1.5 and d == pytest.approx(m["dist"], rel=0.5)     # (each end is rounded to binary32 at 5000: up to 5e-4 off)
        assert 0.1 * m["dist"] <= m["size"] <= 0.5 * m["dist"]
    else:
        assert fam == "shell"
        assert 5.0 <= np.linalg.norm(pos - cc.matrix(sc.instances[cc.ANCHOR_I])[:, 3]) <= 32.0


def _check_light(sc, pose, geom):
    fam, m = pose.families[1], pose.meta["light"]
    p = pose.vec("light_position")
    if fam == "outside":
        assert not any(_in_box(pose, k, p) for k in range(len(pose.instances)) if int(pose.instances[k]["custom_index_and_mask"]) >> 24)
    elif fam == "in_box":
        k = m["inst"]
        assert _in_box(pose, k, p) and not cc.inside_mesh(pose.instances[k], int(pose.instances[k]["mesh"]), p)
    elif fam == "in_mesh":
        assert cc.inside_mesh(pose.instances[m["inst"]], int(pose.instances[m["inst"]]["mesh"]), p)
    elif fam == "near_surface":
        assert m["dist"] in cc.NEAR_SURFACE and _nearest(pose, geom, p) == pytest.approx(m["dist"], rel=0.1)
    elif fam == "on_box_plane":
        w = _corners(pose, m["inst"])
        assert p[m["axis"]] == m["plane"] and m["plane"] in (w[:, m["axis"]].min(), w[:, m["axis"]].max())
        assert not cc.inside_mesh(pose.instances[m["inst"]], int(pose.instances[m["inst"]]["mesh"]), p)
    elif fam == "cube_diagonal":
        d = p[1] - m["floor_y"]
        assert d > 0 and np.all(p * 4 == np.round(p * 4))         # dyadic: the floor points (+-d, -d, +-d) from it are exact ties
        w = _corners(pose, cc.FLOOR_I)
        assert w[:, 0].min() < p[0] - d and p[0] + d < w[:, 0].max() and w[:, 2].min() < p[2] - d and p[2] + d < w[:, 2].max()
    elif fam == "at_camera":
        assert np.array_equal(p, pose.vec("position"))
    elif fam == "far":
        assert np.linalg.norm(p - cc.matrix(sc.instances[cc.ANCHOR_I])[:, 3]) == pytest.approx(1.0e4, rel=1e-3)
    else:
        assert fam == "far_origin" and pose.families[0] == "far_origin_closeup" and np.abs(p).min() >= 280.0


def test_every_case_is_what_its_family_says(cases):
    wrong = []
    for sc, pose, geom, *_ in cases[0]:
        assert (pose.W, pose.H) in cc.FRAME_SIZES or pose.meta["camera"].get("quoted")
        assert np.isfinite(pose.uniforms[0]["position"]).all() and len(pose.instances) <= cc.MAX_INSTANCES
        for check in (_check_camera, _check_light):
            try:
                check(sc, pose, geom)
            except AssertionError as e:
                wrong.append("seed %d: %r\nmeta %r\n%s" % (SEED, pose, pose.meta, str(e)[:400]))
    assert not wrong, "%d cases\n" % len(wrong) + "\n".join(wrong[:10])


def test_the_quoted_close_up_is_among_the_cases(cases):
    q = [p for _, p, *_ in cases[0] if p.meta["camera"].get("quoted")]
    assert len(q) == 1
    p = q[0]
    assert (p.W, p.H, int(p.uniforms[0]["samples_per_pixel"]), len(p.instances)) == (200, 120, 4, 1)
    assert p.vec("position").tolist() == [float(np.float32(x)) for x in (3000.3, -2000.7, 5000.1)]
    M = cc.matrix(p.instances[0])
    assert np.array_equal(M[:, :3], np.diag([float(np.float32(0.002))] * 3))
    assert np.array_equal(M[:, 3].astype(np.float32), (p.vec("position") + (-0.0012, 0.0007, -0.01)).astype(np.float32))


def test_every_family_has_cases_and_they_are_not_empty(cases):
    """per family: at least MIN_CASES cases; at least half of them with primary hits, a third with shadow rays, 4 with secondary rays"""
    fam = {}
    for sc, pose, geom, img, rc, bf, rc_bf, hit_pixels in cases[0]:
        for f in pose.families:
            c = fam.setdefault(f, [0, 0, 0, 0])
            c[0] += 1; c[1] += int(hit_pixels > 0); c[2] += int(rc[2] > 0); c[3] += int(rc[1] > 0)
    assert set(fam) == set(cc.CAMERA_FAMILIES) | set(cc.LIGHT_FAMILIES)
    for f, (n, hits, shadow, secondary) in sorted(fam.items()):
        assert n >= MIN_CASES, (f, n)
        assert 2 * hits >= n, (f, n, hits)
        assert 3 * shadow >= n or f in MAY_LACK_SHADOW_RAYS, (f, n, shadow)
        assert secondary >= 4, (f, n, secondary)


def test_the_oracle_can_referee_every_case(cases):
    """finite frames (at most 2 % of the draws replaced for that), and tree mode == brute-force mode bit for bit with equal ray counts"""
    all_cases, refused = cases
    assert len(refused) <= 0.02 * len(all_cases), refused
    assert sum(p.replaced for _, p, *_ in all_cases) == len(refused)
    for sc, pose, geom, img, rc, bf, rc_bf, _ in all_cases:
        assert np.isfinite(img).all(), pose
        assert np.array_equal(img.view(np.uint32), bf.view(np.uint32)) and np.array_equal(rc, rc_bf), \
            "seed %d: %r: the oracle's tree mode and its brute force differ in %d pixels, rays %s / %s" % (
                SEED, pose, int((img.view(np.uint32) != bf.view(np.uint32)).any(axis=2).sum()), rc.tolist(), rc_bf.tolist())
