"""Seeded adversarial inputs for the frame path's conservative culls (k_cover's coverage mask, k_entry's camera- and light-side entry
records, k_beam's pixel beams, the settled shadow rays): scenes(seed) yields the scenes, poses(scene, seed) the (camera, light, W, H)
cases of one scene, each tagged with the families it belongs to.  tests/test_cull_cases.py checks on the CPU that every case is what
its family says (binary64 predicates over the binary32 inputs) and that the oracle can referee it; tests/test_cull_fuzz.py renders
them on the GPU with every cull off, on, and one at a time.

A case is self-contained: its own instance records, per-instance types and uniform block (a close-up far from the origin translates
the whole scene; a sub-pixel object is an instance of its own), over the scene's five meshes.  No GPU and no torch in here."""
import os
import tempfile

import numpy as np

DEFAULT_SEED = 20261020
N_SCENES = 12
N_POSES = 16
MAX_INSTANCES = 8             # a scene has 4-6 instances and a case adds at most one; the type table is this long
KF = 2.5                      # src/shader.rgen:79: d = ux right + uy up + 2.5 forward
APEX_RADIUS = 0.0102          # rt_api.cpp: the light-side beams are widened by this
FRAME_SIZES = ((8, 8), (9, 7), (64, 40), (96, 64), (203, 117))
CAMERA_FAMILIES = ("shell", "in_box", "in_mesh", "on_box_plane", "axis_view", "grazing", "wide", "long_lens", "left_handed",
                   "near_singular", "subpixel_on_tile_corner", "off_screen_edge", "far_origin_closeup")
LIGHT_FAMILIES = ("outside", "in_box", "in_mesh", "near_surface", "on_box_plane", "cube_diagonal", "at_camera", "far", "far_origin")
NEAR_SURFACE = (0.005, 0.0102, 0.02, 0.05)
MESHES = ("cube", "teapot", "floor", "sliver", "octahedron")
CUBE, TEAPOT, FLOOR, SLIVER, OCTA = range(5)
# object-space boxes of the meshes (tests/test_cull_cases.py checks them against the loaded geometry)
MESH_LO = np.array([(-1, -1, -1), (-3.0, 0.0, -2.0), (-1, 0, -1), (-1, 0, -1e-3), (-1, -1, -1)], np.float64)
MESH_HI = np.array([(1, 1, 1), (3.42963, 3.15, 2.0), (1, 0, 1), (1, 0, 1e-3), (1, 1, 1)], np.float64)
FLOOR_I, ANCHOR_I, TILTED_I = 0, 1, 2   # instance 0: the floor; 1: an axis-aligned cube / octahedron; 2: a rotated cube / octahedron


def _quad(x, z):
    v = np.zeros((4, 6), np.float32)
    v[:, 0] = (-x, x, x, -x); v[:, 2] = (-z, -z, z, z); v[:, 4] = 1.0
    return v, np.array([0, 2, 1, 0, 3, 2], np.uint32)


def _octahedron():
    p = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float32)
    v = np.concatenate([p, p], axis=1)          # (vertex normals: the direction of the vertex)
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return v, np.array(f, np.uint32).reshape(-1)


_MESH_DIR = []


def mesh_paths(directory=None):
    """the five meshes' OBJ files, in MESHES order (floor, sliver plate and octahedron are written on first use)"""
    from tests import scenes as sc
    if directory is None:
        if not _MESH_DIR:
            _MESH_DIR.append(tempfile.mkdtemp(prefix="cull_cases_"))
        directory = _MESH_DIR[0]
    made = {"floor": _quad(1.0, 1.0), "sliver": _quad(1.0, 1e-3), "octahedron": _octahedron()}
    paths = []
    for name in MESHES:
        if name in made:
            p = os.path.join(directory, name + ".obj")
            if not os.path.exists(p):
                sc.write_obj(p, *made[name])
            paths.append(p)
        else:
            paths.append(os.path.join(sc.RES, name + ".obj"))
    return paths


class Scene:
    """paths, instances (INSTANCE_DTYPE), types (uint32 per instance, MAX_INSTANCES long: shared by every case of the scene), uniforms
    (UNIFORMS_DTYPE (1,)) and sky: the ScenePair inputs, and what poses() places its cameras and lights against"""

    def __init__(self, index, seed, paths, instances, types, uniforms, sky):
        self.index, self.seed, self.paths, self.instances, self.types, self.uniforms, self.sky = index, seed, paths, instances, types, uniforms, sky
        self.name = "scene%02d" % index

    @property
    def mesh_of(self):
        return [int(m) for m in self.instances["mesh"]]


class Pose:
    """one case: instances / types / uniforms (camera, light, samples, bounces) and the frame size; families = (camera family,
    light family); meta: what the family's predicate needs (the instance it refers to, the intended distance, ...)"""

    def __init__(self, name, families, instances, types, uniforms, W, H, meta):
        self.name, self.families, self.instances, self.types, self.uniforms, self.W, self.H, self.meta = name, families, instances, types, uniforms, W, H, meta
        self.replaced = 0       # how many draws of this case were refused by poses()'s `accept` before this one

    def vec(self, field):
        return np.asarray(self.uniforms[0][field][:3], np.float64)

    def __repr__(self):
        return "%s %s %dx%d cam %s light %s" % (self.name, "/".join(self.families), self.W, self.H, self.vec("position").tolist(), self.vec("light_position").tolist())


# ---- small linear algebra (binary64; records and uniforms are rounded to binary32 when they are stored) ----------------------------
def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _rot(axis, ang):
    a = _unit(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)


def matrix(record):
    """3x4 float64 of an instance record's binary32 transform"""
    return np.asarray(record["transform"], np.float64).reshape(3, 4)


def world_box(record, mesh):
    """AABB of the instance's transformed object box (binary64 over the binary32 record)"""
    M = matrix(record)
    c = np.array([[(MESH_HI if (k >> a) & 1 else MESH_LO)[mesh][a] for a in range(3)] for k in range(8)])
    w = c @ M[:, :3].T + M[:, 3]
    return w.min(0), w.max(0)


def inside_mesh(record, mesh, p):
    """binary64: is the world point strictly inside the closed mesh (cube / octahedron) of the instance?"""
    M = matrix(record)
    q = np.linalg.solve(M[:, :3], np.asarray(p, np.float64) - M[:, 3])
    return bool(np.abs(q).max() < 1.0) if mesh == CUBE else bool(np.abs(q).sum() < 1.0)


def look(pos, target, roll=0.0):
    """orthonormal right, up, forward of a camera at pos that looks at target"""
    f = _unit(np.asarray(target, np.float64) - pos)
    h = np.array([0.0, 1.0, 0.0]) if abs(f[1]) < 0.95 else np.array([1.0, 0.0, 0.0])
    r = _unit(np.cross(f, h)); u = np.cross(r, f)
    c, s = np.cos(roll), np.sin(roll)
    return c * r + s * u, c * u - s * r, f


def project(pose, p):
    """binary64 pixel coordinates and depth (px, py, az) of a world point: (a, b, c) = basis^-1 (p - cam), ux = KF a / c"""
    B = np.stack([pose.vec("right"), pose.vec("up"), pose.vec("forward")], axis=1)
    a = np.linalg.solve(B, np.asarray(p, np.float64) - pose.vec("position"))
    with np.errstate(all="ignore"):
        return (KF * a[0] / a[2] + 1) * 0.5 * pose.W, (1 - KF * a[1] / a[2]) * 0.5 * pose.H, a[2]


def camera_det_ratio(pose):
    """|det| of the camera basis over rt_api.cpp's threshold 1e-6 scale^3 / 27 (the coverage mask refuses a basis at or below 1)"""
    B = np.stack([pose.vec("right"), pose.vec("up"), pose.vec("forward")], axis=1)
    return abs(np.linalg.det(B)) / (1e-6 * np.abs(B).sum() ** 3 / 27.0)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def _record(M, t, obj_index, mesh, mask=0xFF):
    from vulkan_raytracing_amd import host
    r = host.make_instance(np.concatenate([M, np.asarray(t, np.float64)[:, None]], axis=1).astype(np.float32).reshape(12), obj_index, mesh)
    if mask != 0xFF:
        r["custom_index_and_mask"] = (int(r["custom_index_and_mask"]) & 0x00FFFFFF) | (mask << 24)
    return r


def _random_linear(rng, lo, hi, k):
    """rotation x non-uniform scale in [lo, hi] (log-uniform), with shear (k % 3 == 1) or mirroring (k % 3 == 2)"""
    M = _rot(rng.normal(size=3), rng.uniform(0.5, 1.0) * rng.choice([-1, 1])) @ np.diag(np.exp(rng.uniform(np.log(lo), np.log(hi), size=3)))
    if k % 3 == 1:
        M = M @ np.array([[1.0, rng.uniform(-0.6, 0.6), 0.0], [0.0, 1.0, 0.0], [rng.uniform(-0.4, 0.4), 0.0, 1.0]])
    elif k % 3 == 2:
        M = M @ np.diag([-1.0, 1.0, 1.0])
    return M


def scenes(seed=DEFAULT_SEED, n=N_SCENES, directory=None):
    """n scenes of 4-6 instances over the five meshes: [0] the floor (one quad scaled to 40 x 40, diffuse, the shadow receiver), [1] an
    axis-aligned cube or octahedron with dyadic scale and position (its box planes are exact in binary32), [2] a rotated cube or
    octahedron, then a teapot or sliver plate or two, and last a big cube with mask 0 around the others that no ray may see.  Scales
    0.05 .. 20; shear or mirroring in a third of the transforms; a mirror and a glass instance in every scene."""
    from tests import scenes as sc
    from vulkan_raytracing_amd import host
    from vulkan_raytracing_amd.api import INSTANCE_DTYPE
    paths = mesh_paths(directory)
    geom = host.SceneGeometry(paths)
    sky = sc.synthetic_skybox(64)
    for index in range(n):
        rng = np.random.default_rng([seed, index])
        fy = -2.0
        recs = [_record(np.diag([20.0, 1.0, 20.0]), (0.0, fy, 0.0), 0, FLOOR)]
        s = rng.choice([0.5, 0.75, 1.0, 1.5, 2.0], size=3)
        recs.append(_record(np.diag(s), (rng.integers(-8, 9) * 0.25, fy + s[1] + 0.25, rng.integers(-8, 9) * 0.25), 1, int(rng.choice([CUBE, OCTA]))))
        recs.append(_record(_random_linear(rng, 0.3, 2.5, index), (rng.uniform(-5, 5), fy + rng.uniform(2.5, 4.0), rng.uniform(-5, 5)), 1, int(rng.choice([CUBE, OCTA]))))
        for k in range(int(rng.integers(1, 3))):
            mesh = TEAPOT if k == 0 and index % 4 != 3 else int(rng.choice([SLIVER, SLIVER, TEAPOT, CUBE]))
            lo, hi = ((0.05, 1.0), (0.5, 20.0), (0.05, 3.0))[(TEAPOT, SLIVER, CUBE).index(mesh)]
            recs.append(_record(_random_linear(rng, lo, hi, index + k + 1), (rng.uniform(-6, 6), fy + rng.uniform(0.5, 4.0), rng.uniform(-6, 6)), 1, mesh))
        recs.append(_record(np.diag(rng.uniform(3.0, 6.0, size=3)), matrix(recs[ANCHOR_I])[:, 3] + rng.uniform(-1, 1, size=3), 1, CUBE, mask=0))
        types = np.zeros(MAX_INSTANCES, np.uint32)                   # (an instance a case adds is diffuse: it casts and receives shadows)
        types[1:3] = rng.permutation([1, 2])                         # a mirror and a glass instance (1 mirror, 2 refractive)
        types[3:len(recs)] = rng.integers(0, 3, size=len(recs) - 3)
        u = host.default_uniforms(max_bounce_count=int(rng.integers(0, 4)), samples_per_pixel=int(rng.choice([1, 2, 4, 5])),
                                  orbiting_object_primitive_offset=geom.orbiting_primitive_offset, orbiting_object_vertex_offset=geom.orbiting_vertex_offset)
        yield Scene(index, seed, paths, np.asarray(recs, INSTANCE_DTYPE), types, u, sky)


# ---- cameras --------------------------------------------------------------------------------------------------------------------------
def _corner_point(rng, scene, k, frac=0.06):
    """a point inside the world box of instance k and outside its (closed) mesh: near a corner of the box"""
    lo, hi = world_box(scene.instances[k], scene.mesh_of[k])
    for _ in range(64):
        side = rng.integers(0, 2, size=3)
        p = np.where(side, hi - frac * (hi - lo), lo + frac * (hi - lo)).astype(np.float32).astype(np.float64)
        if not inside_mesh(scene.instances[k], scene.mesh_of[k], p):
            return p
    raise AssertionError("no box corner of instance %d lies outside its mesh" % k)


def _center(scene, k):
    lo, hi = world_box(scene.instances[k], scene.mesh_of[k])
    return 0.5 * (lo + hi), 0.5 * (hi - lo)


def _shell(rng, scene):
    c, _ = _center(scene, ANCHOR_I)
    d = _unit(rng.normal(size=3)); d[1] = abs(d[1]) * 0.7 + 0.05
    pos = c + _unit(d) * rng.uniform(6.0, 30.0)
    return pos, look(pos, c + rng.uniform(-2.0, 2.0, size=3), rng.uniform(-0.4, 0.4))


def _camera(rng, scene, family, variant, W, H):
    """(position, (right, up, forward), meta, extra instance records, translation of the whole case)"""
    meta, extra, shift = {}, [], None
    c, h = _center(scene, ANCHOR_I)
    if family == "shell":
        pos, basis = _shell(rng, scene)
    elif family == "in_box":
        pos = _corner_point(rng, scene, TILTED_I); meta["inst"] = TILTED_I
        basis = look(pos, _center(scene, TILTED_I)[0] if variant % 2 else c, rng.uniform(-0.3, 0.3))
    elif family == "in_mesh":
        pos = c + rng.uniform(-0.25, 0.25, size=3) * h * (1.0 if scene.mesh_of[ANCHOR_I] == CUBE else 0.5); meta["inst"] = ANCHOR_I
        basis = look(pos, pos + _unit(rng.normal(size=3)), rng.uniform(-0.3, 0.3))
    elif family == "on_box_plane":
        # coordinate `axis` exactly on a face plane of the anchor's world box, beside the face; forward = -+e_axis looks across the
        # box's slab (four corners at depth exactly 0), or along the plane (variant 2)
        axis, sgn = int(rng.integers(0, 3)), int(rng.choice([-1, 1]))
        if axis == 1:
            sgn = 1           # (the plane under the anchor runs a quarter unit above the floor: stay on top)
        pos = c + rng.uniform(-0.5, 0.5, size=3) * h
        pos[axis] = c[axis] + sgn * h[axis]
        side = (axis + 1 + int(rng.integers(0, 2))) % 3
        if side == 1:
            side = (axis + 1) % 3 if (axis + 1) % 3 != 1 else (axis + 2) % 3
        pos[side] = c[side] + rng.choice([-1, 1]) * (h[side] + rng.uniform(0.25, 1.0))
        f = np.zeros(3)
        if variant % 3 == 2:
            f[side] = -np.sign(pos[side] - c[side])
        else:
            f[axis] = -sgn if variant % 3 == 0 else sgn
        r = np.zeros(3); r[3 - axis - side] = 1.0
        basis = (r, np.cross(r, f), f)
        meta.update(inst=ANCHOR_I, axis=axis, plane=float(np.float32(c[axis] + sgn * h[axis])))
    elif family == "axis_view":
        k, sgn = int(rng.integers(0, 3)), int(rng.choice([-1, 1]))
        f = np.zeros(3); f[k] = sgn
        r = np.zeros(3); r[(k + 1) % 3] = rng.choice([-1, 1])
        pos = c - f * rng.uniform(4.0, 12.0) + rng.uniform(-1.0, 1.0, size=3)
        if k == 1 and sgn > 0:
            pos[1] = c[1] - h[1] - 0.1      # looking up from between the floor and the anchor
        basis = (r, np.cross(r, f) * rng.choice([-1, 1]), f)
    elif family == "grazing":
        ang = 10.0 ** rng.uniform(-4, -2)
        meta.update(angle=ang)
        if variant % 2 == 0:       # along the floor, towards the anchor, from just above it
            fy = matrix(scene.instances[FLOOR_I])[1, 3]
            a = rng.uniform(0, 2 * np.pi)
            pos = np.array([c[0] + 9.0 * np.cos(a), fy + rng.uniform(0.002, 0.05), c[2] + 9.0 * np.sin(a)])
            flat = _unit([c[0] - pos[0], 0.0, c[2] - pos[2]])
            f = np.cos(ang) * flat - np.sin(ang) * np.array([0.0, 1.0, 0.0])
            meta.update(normal=[0.0, 1.0, 0.0])
        else:                      # along a side plane of the anchor's box, from just outside it
            axis = int(rng.choice([0, 2])); other = 2 - axis
            n = np.zeros(3); n[axis] = rng.choice([-1, 1])
            t = np.zeros(3); t[other] = 1.0
            pos = c + n * (h[axis] + rng.uniform(0.002, 0.05)) - t * (h[other] + 4.0)
            f = np.cos(ang) * t - np.sin(ang) * n
            meta.update(normal=n.tolist())
        r = _unit(np.cross(f, meta["normal"]))
        basis = (r, np.cross(r, f), f)
    elif family in ("wide", "long_lens"):
        pos, (r, u, f) = _shell(rng, scene)
        if family == "long_lens":
            pos = c + _unit(pos - c) * rng.uniform(30.0, 80.0)
            # (aimed at the anchor, or at a corner of the tilted instance's box, where the box is empty and its mesh begins)
            aim = _corner_point(rng, scene, TILTED_I, frac=0.2) if variant % 2 else c + rng.uniform(-0.5, 0.5, size=3) * h
            r, u, f = look(pos, aim, rng.uniform(-0.4, 0.4))
        meta.update(forward_scale=0.1 if family == "wide" else 50.0)
        basis = (r * rng.uniform(0.6, 0.9), u * rng.uniform(1.1, 1.6), f * meta["forward_scale"])
    elif family == "left_handed":
        pos, (r, u, f) = _shell(rng, scene)
        basis = (-r, u, f) if variant % 2 else (r, -u, f)      # (the reference's camera has right x up = -forward, det -1: this one det +1)
    elif family == "near_singular":
        # right = a up + eps e (e perpendicular to up and forward, all three along axes): det = +-eps exactly
        ratio = 2.0 if variant % 2 else 0.5
        k = int(rng.integers(0, 3)); sgn = int(rng.choice([-1, 1]))
        f = np.zeros(3); f[k] = sgn
        u = np.zeros(3); u[(k + 1) % 3] = 1.0
        e = np.zeros(3); e[(k + 2) % 3] = 1.0
        a = rng.uniform(0.5, 1.0); eps = 0.0
        for _ in range(8):
            eps = ratio * 1e-6 * (2.0 + a + eps) ** 3 / 27.0
        basis = (a * u + eps * e, u, f)
        pos = c - f * rng.uniform(4.0, 9.0) + rng.uniform(-0.3, 0.3, size=3) * h
        meta.update(ratio=ratio)
    elif family == "subpixel_on_tile_corner":
        pos, basis = _shell(rng, scene)
        pos = c + _unit(pos - c) * rng.uniform(5.0, 9.0)
        basis = look(pos, c, rng.uniform(-0.2, 0.2))
        s = 10.0 ** rng.uniform(-3, -2)
        if variant % 3 == 2 or W < 16:     # the frame's corner
            px, py = float(rng.choice([0, W])), float(rng.choice([0, H]))
        else:                              # a point where four 8x8 tiles meet
            px, py = 8.0 * rng.integers(1, (W + 7) // 8), 8.0 * rng.integers(1, (H + 7) // 8)
            px, py = min(px, 8.0 * (W // 8)), min(py, 8.0 * (H // 8))
        r, u, f = (np.asarray(v, np.float32).astype(np.float64) for v in basis)
        pos = pos.astype(np.float32).astype(np.float64)
        d = (2.0 * px / W - 1.0) * r + (1.0 - 2.0 * py / H) * u + KF * f
        depth = 2.0 * s * W * KF / (2.0 * 0.6)          # the object's extent 2 s spans 0.6 of a pixel: a pixel at depth c is 2 c / (KF W) wide
        mesh = int(rng.choice([CUBE, OCTA]))
        extra.append((_random_linear(rng, s, s, 0), pos + d * (depth / KF), mesh))
        meta.update(pixel=(px, py), scale=s, inst=len(scene.instances))
    elif family == "off_screen_edge":
        d = _unit(rng.normal(size=3)); d[1] = abs(d[1])
        pos = c + _unit(d) * float(np.linalg.norm(h)) * rng.uniform(2.0, 4.0)
        r, u, f = look(pos, c, rng.uniform(-0.3, 0.3))
        dist = float(np.linalg.norm(c - pos))
        if variant % 3 == 2:       # the box straddles the camera plane: its centre at depth 0
            f2 = _unit(np.cross(c - pos, u)); basis = (np.cross(u, f2), u, f2)
            meta.update(kind="camera_plane")
        else:                      # its centre on a frame edge (ux = +-1), or on a corner (and uy = +-1)
            ux, uy = float(rng.choice([-1, 1])), (float(rng.choice([-1, 1])) if variant % 3 == 1 else float(rng.uniform(-0.5, 0.5)))
            f2 = _unit(KF * f - ux * r - uy * u)       # turn the camera so that the old centre ray leaves through (ux, uy)
            r2 = _unit(np.cross(f2, u)); basis = (r2, np.cross(r2, f2), f2)
            meta.update(kind="corner" if variant % 3 == 1 else "edge")
        meta.update(inst=ANCHOR_I, dist=dist)
    elif family == "far_origin_closeup":
        # the whole case moved by 300 / 1000 / 5000 per axis; the camera 0.003 .. 0.02 in front of a small object (0.15 .. 0.5 of that)
        pos, basis = _shell(rng, scene)
        shift = float(rng.choice([300.0, 1000.0, 5000.0])) * rng.choice([-1.0, 1.0], size=3)
        dist = 10.0 ** rng.uniform(np.log10(0.003), np.log10(0.02))
        size = dist * rng.uniform(0.15, 0.5)
        r, u, f = basis
        at = pos + dist * _unit(KF * f + rng.uniform(-0.6, 0.6) * r + rng.uniform(-0.6, 0.6) * u) + 0.0
        mesh = int(rng.choice([CUBE, OCTA]))
        M = np.diag([size, size, size]) if variant % 2 else _random_linear(rng, 0.5 * size, size, variant)
        extra.append((M, at, mesh))
        meta.update(shift=shift.tolist(), dist=dist, size=size, inst=len(scene.instances))
    else:
        raise ValueError(family)
    return np.asarray(pos, np.float64), basis, meta, extra, shift


# ---- lights ---------------------------------------------------------------------------------------------------------------------------
def _surface_point(rng, scene, k):
    """a point well inside a triangle of instance k (floor, cube or octahedron) and the triangle's unit normal, in world space"""
    mesh = scene.mesh_of[k]
    if mesh == FLOOR:
        q, n = np.array([rng.uniform(-0.3, 0.3), 0.0, rng.uniform(-0.3, 0.3)]), np.array([0.0, 1.0, 0.0])
    elif mesh == CUBE:        # a face of the cube, away from its edges and from the diagonal that splits it
        a = int(rng.integers(0, 3)); s = float(rng.choice([-1, 1]))
        q = np.zeros(3); q[a] = s; q[(a + 1) % 3] = rng.uniform(0.3, 0.6) * rng.choice([-1, 1]); q[(a + 2) % 3] = rng.uniform(0.05, 0.15) * rng.choice([-1, 1])
        n = np.zeros(3); n[a] = s
    else:                     # a face of the octahedron: x / sx + y / sy + z / sz = 1, near its centroid
        sg = rng.choice([-1.0, 1.0], size=3)
        w = rng.uniform(0.25, 0.4, size=2)
        q = sg * np.array([w[0], w[1], 1.0 - w.sum()]); n = sg / np.sqrt(3.0)
    M = matrix(scene.instances[k])
    wn = _unit(np.linalg.inv(M[:, :3]).T @ n)
    return M[:, :3] @ q + M[:, 3], wn


def _light(rng, scene, family, variant, cam_pos):
    meta = {}
    c, h = _center(scene, ANCHOR_I)
    fy = matrix(scene.instances[FLOOR_I])[1, 3]
    if family == "outside":
        for _ in range(64):
            p = rng.uniform(-15.0, 15.0, size=3); p[1] = fy + abs(p[1]) + 1.0
            if not any(np.all(p >= lo) and np.all(p <= hi) for lo, hi in (world_box(r, m) for r, m in zip(scene.instances, scene.mesh_of))):
                break
    elif family == "in_box":
        p = _corner_point(rng, scene, TILTED_I, frac=rng.uniform(0.03, 0.15)); meta["inst"] = TILTED_I
    elif family == "in_mesh":
        p = c + rng.uniform(-0.25, 0.25, size=3) * h * (1.0 if scene.mesh_of[ANCHOR_I] == CUBE else 0.5); meta["inst"] = ANCHOR_I
    elif family == "near_surface":
        k = (FLOOR_I, ANCHOR_I, TILTED_I)[variant % 3]
        d = NEAR_SURFACE[(variant // 3) % 4]
        q, n = _surface_point(rng, scene, k)
        p = q + n * d * (1.0 if (variant // 12) % 2 == 0 else -1.0)
        meta.update(inst=k, dist=d)
    elif family == "on_box_plane":
        axis, sgn = int(rng.integers(0, 3)), int(rng.choice([-1, 1]))
        if axis == 1:
            sgn = 1
        p = c + rng.uniform(-1.5, 1.5, size=3) * h
        p[axis] = c[axis] + sgn * h[axis]
        side = (axis + 1) % 3 if (axis + 1) % 3 != 1 else (axis + 2) % 3
        p[side] = c[side] + rng.choice([-1, 1]) * (h[side] + rng.uniform(0.1, 2.0))
        p[1] = max(p[1], fy + 0.25)
        meta.update(inst=ANCHOR_I, axis=axis, plane=float(np.float32(c[axis] + sgn * h[axis])))
    elif family == "cube_diagonal":
        # dyadic light over the floor at a dyadic height: the floor points at (+-d, -d, +-d) from it are on the light cube's corners,
        # those at (+-d, -d, z) on its edges; variant 1: the anchor's centre on a corner diagonal as well
        d = float(rng.integers(8, 33)) * 0.25
        p = np.array([rng.integers(-16, 17) * 0.25, fy + d, rng.integers(-16, 17) * 0.25])
        if variant % 2:
            sg = rng.choice([-1.0, 1.0], size=3); sg[1] = 1.0
            e = float(rng.integers(4, 13)) * 0.5
            p = np.round(c * 4.0) / 4.0 + sg * e
        meta.update(floor_y=float(fy))
    elif family == "at_camera":
        p = np.asarray(cam_pos, np.float64).copy()
    elif family == "far":
        d = _unit(rng.normal(size=3)); d[1] = abs(d[1]) + 0.2
        p = c + _unit(d) * 1.0e4
    elif family == "far_origin":
        p = c + np.array([rng.uniform(-6, 6), rng.uniform(3, 10), rng.uniform(-6, 6)])
    else:
        raise ValueError(family)
    return np.asarray(p, np.float64), meta


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
def _assemble(scene, name, families, W, H, pos, basis, light, meta, extra, shift, hide_floor):
    from vulkan_raytracing_amd.api import INSTANCE_DTYPE
    inst = scene.instances.copy()
    if hide_floor:      # mask 0: the floor's one box reaches behind most cameras, and k_cover then marks the whole frame
        inst["custom_index_and_mask"][FLOOR_I] &= 0x00FFFFFF
    if extra:
        recs = [_record(M, t, 1, mesh) for M, t, mesh in extra]
        inst = np.concatenate([inst, np.asarray(recs, INSTANCE_DTYPE)])
    if shift is not None:      # every translation, the camera and the light move together (each rounded to binary32 on its own)
        T = inst["transform"].astype(np.float64).reshape(-1, 3, 4)
        T[:, :, 3] += shift
        inst["transform"] = T.reshape(-1, 12).astype(np.float32)
        pos = pos + shift; light = light + shift
    u = scene.uniforms.copy()
    u[0]["position"][:3] = pos; u[0]["right"][:3] = basis[0]; u[0]["up"][:3] = basis[1]; u[0]["forward"][:3] = basis[2]
    u[0]["light_position"][:3] = light
    return Pose(name, families, inst, scene.types, u, W, H, meta)


def quoted_closeup(scene):
    """the fixed case of the issue that first put k_cover's margin in doubt: the +-1 cube scaled by 0.002, a hundredth of a unit in
    front of a camera at (3000.3, -2000.7, 5000.1) that looks down -z; 200 x 120 pixels, 4 samples, nothing else in the scene"""
    from vulkan_raytracing_amd.api import INSTANCE_DTYPE
    cam = np.array([3000.3, -2000.7, 5000.1], np.float32)
    t = (cam.astype(np.float64) + (-0.0012, 0.0007, -0.01)).astype(np.float32)
    inst = np.asarray([_record(np.diag([0.002] * 3), t.astype(np.float64), 0, CUBE)], INSTANCE_DTYPE)
    u = scene.uniforms.copy()
    u[0]["samples_per_pixel"] = 4
    u[0]["position"][:3] = cam; u[0]["right"][:3] = (1, 0, 0); u[0]["up"][:3] = (0, 1, 0); u[0]["forward"][:3] = (0, 0, -1)
    u[0]["light_position"][:3] = cam.astype(np.float64) + (0.5, 2.0, 1.0)
    meta = dict(camera=dict(shift=cam.astype(np.float64).tolist(), dist=0.01, size=0.002, inst=0, quoted=True), light={}, floor_hidden=False)
    return Pose(scene.name + "/quoted_closeup", ("far_origin_closeup", "far_origin"), inst, scene.types, u, 200, 120, meta)


def poses(scene, seed=DEFAULT_SEED, n=N_POSES, accept=None):
    """n cases of the scene (scene 0: plus the quoted close-up).  Case i takes camera family (i + scene) mod 13 and one of the first
    eight light families, shifted per scene so that every pair meets; far_origin_closeup cameras take the far_origin light.
    A third of the cases hide the floor (mask 0), where neither family needs it: its single box reaches behind most cameras.
    accept(pose) -> bool: a case the caller cannot use (the oracle's frame is not finite: a sample landed on the light) is drawn
    again from the next sub-seed, and pose.replaced counts the draws that were refused."""
    for i in range(n):
        cam_family = CAMERA_FAMILIES[(i + scene.index) % len(CAMERA_FAMILIES)]
        light_family = "far_origin" if cam_family == "far_origin_closeup" else LIGHT_FAMILIES[(i * 3 + scene.index + i // 8) % 8]
        variant = scene.index + (i // len(CAMERA_FAMILIES))
        for attempt in range(8):
            rng = np.random.default_rng([seed, scene.index, i, attempt])
            W, H = FRAME_SIZES[int(rng.integers(0, len(FRAME_SIZES)))]
            if cam_family == "shell" and (W, H) == (203, 117):
                W, H = 96, 64              # (the control family stays cheap)
            pos, basis, meta, extra, shift = _camera(rng, scene, cam_family, variant, W, H)
            light, lmeta = _light(rng, scene, light_family, scene.index * N_POSES + i, pos)
            # a third of the cases (two thirds of the close-ups far from the origin) without the floor, where no case needs it
            hide_floor = ((i + scene.index) % 3 == 1 or (cam_family == "far_origin_closeup" and (i + scene.index) % 3 == 2)) and \
                cam_family != "grazing" and light_family not in ("near_surface", "cube_diagonal")
            meta = dict(camera=meta, light=lmeta, floor_hidden=hide_floor)
            p = _assemble(scene, "%s/pose%02d" % (scene.name, i), (cam_family, light_family), W, H, pos, basis, light, meta, extra, shift, hide_floor)
            p.replaced = attempt
            if accept is None or accept(p):
                break
        else:
            raise AssertionError("no usable draw for %r" % p)
        yield p
    if scene.index == 0:
        yield quoted_closeup(scene)
