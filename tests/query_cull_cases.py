"""Seeded adversarial inputs for the conservative culls of the record-level world-space queries (closest point and its K nearest form,
box and triangle overlaps, sphere sweeps, closest segments and triangles): scenes(seed) yields the scenes, each instance tagged with
its families, and point_records / sweep_records / box_records / segment_records / triangle_records place query records against one
scene in binary64 and round them to binary32, each set tagged with its record family.  tests/test_query_cull_cases.py checks on the
CPU that every instance is what its family says and that the brute-force references alone can referee the records;
tests/test_query_cull_fuzz.py runs them on the GPU against those references byte for byte.

What the culls have to survive: instances of condition 10 to 1000 and shears of sigma_min / sigma_max near 1e-3 over
a mesh of 640 triangles (a BLAS eight or more levels deep, so that pruning happens inside the instance), uniform scales 1e-3 and 1e3,
object-space offsets of thousands that the translation cancels, coincident and nested instances, a flat record, a NaN record, and three
scenes translated as a whole by 1e3, 1e4 and 1e5.  rt_api.h excludes needles "of aspect 1e-4 and below" from tree independence: every
world triangle of an instance that is neither singular nor void is held at ASPECT_FLOOR = 1e-3, ten times that limit (aspect =
2 area / longest_edge^2 in binary64); a draw that fails the floor is repeated with half the condition number.

No GPU and no torch in here."""
import numpy as np

from tests import cull_cases as cc

DEFAULT_SEED = 20261020
N_SCENES = 8
N_RECORDS = 128                # records per record family and query
ASPECT_FLOOR = 1e-3
SCENE_SHIFT = {5: 1.0e3, 6: 1.0e4, 7: 1.0e5}       # the whole scene translated along (1, 1, 1)
INSTANCE_FAMILIES = ("rigid_dyadic", "anisotropic", "sheared", "mirrored", "tiny", "huge", "cancelling", "coincident", "nested", "masked",
                     "singular", "void")
POINT_FAMILIES = ("near_surface", "on_feature", "volume", "far", "box_corner", "equidistant")
# mesh slots of every scene (the vertex and index arrays hold them in this order)
CUBE, OCTA, SOUP, LARGE, LARGE_FAR, LARGE_K, LARGE_M, SOUP_FAR = range(8)
MESHES = ("cube", "octahedron", "soup", "large", "large_far", "large_k", "large_m", "soup_far")
LARGE_MESHES = (LARGE, LARGE_FAR, LARGE_K, LARGE_M)
TORUS_U, TORUS_V = 32, 10      # 2 * 32 * 10 = 640 near-equilateral triangles: rows staggered by half a cell

# (family, mesh, parameter) per scene; every scene ends with the enclosing cube of mask 0.  parameter: the condition number of
# anisotropic / cancelling, "m" adds the mirrored tag, "o" (tiny / huge): the world size stays ordinary (LARGE_K, LARGE_M).
_PLAN = (
    (("anisotropic", LARGE, 1000), ("rigid_dyadic", LARGE, 0), ("cancelling", LARGE_FAR, 100), ("sheared", OCTA, 0), ("tiny", CUBE, 0),
     ("anisotropic", SOUP, "10m"), ("nested", OCTA, 0)),
    (("sheared", LARGE, 0), ("coincident", LARGE, 0), ("rigid_dyadic", CUBE, 0), ("anisotropic", SOUP, 100), ("singular", OCTA, 0),
     ("huge", OCTA, 0)),
    (("tiny", LARGE_K, "o"), ("singular", LARGE, 0), ("anisotropic", LARGE, "1000m"), ("rigid_dyadic", OCTA, 0), ("cancelling", SOUP_FAR, 100),
     ("coincident", CUBE, 0), ("void", CUBE, 0)),
    (("huge", LARGE_M, "o"), ("void", LARGE, 0), ("rigid_dyadic", CUBE, 0), ("nested", LARGE, 0), ("anisotropic", OCTA, 1000),
     ("sheared", SOUP, "m"), ("tiny", OCTA, 0)),
    (("cancelling", LARGE_FAR, 10), ("sheared", LARGE, "m"), ("rigid_dyadic", LARGE, "m"), ("huge", CUBE, 0), ("singular", SOUP, 0),
     ("nested", OCTA, 0), ("anisotropic", CUBE, 100)),
    (("coincident", LARGE, 0), ("anisotropic", LARGE, 100), ("rigid_dyadic", OCTA, 0), ("void", OCTA, 0), ("cancelling", SOUP_FAR, 100),
     ("sheared", CUBE, 0)),
    (("tiny", LARGE_K, "o"), ("singular", LARGE, 0), ("rigid_dyadic", CUBE, 0), ("nested", LARGE, 0), ("coincident", OCTA, 0),
     ("anisotropic", SOUP, 1000)),
    (("huge", LARGE_M, "o"), ("void", LARGE, 0), ("anisotropic", LARGE, 10), ("rigid_dyadic", OCTA, 0), ("sheared", OCTA, 0),
     ("cancelling", SOUP_FAR, "10m")),
)


class Scene:
    """verts, idx, ranges (the upload_geometry arguments), instances (INSTANCE_DTYPE) and per instance: families (a tuple of tags, the
    first the primary one) and meta (the condition number aimed at and drawn, the host of a nested instance, the twin of a coincident
    one, ...); shift: the translation of the whole scene"""

    def __init__(self, index, seed, verts, idx, ranges, instances, families, meta, shift):
        self.index, self.seed, self.verts, self.idx, self.ranges, self.instances = index, seed, verts, idx, ranges, instances
        self.families, self.meta, self.shift = families, meta, shift
        self.name = "scene%02d" % index

    @property
    def parts(self):
        return self.verts, self.idx, self.ranges, self.instances

    def mesh_of(self, i):
        return int(self.instances[i]["mesh"])

    def mask_of(self, i):
        return int(self.instances[i]["custom_index_and_mask"]) >> 24

    def with_family(self, family, large=None):
        return [i for i, f in enumerate(self.families) if family in f and (large is None or (self.mesh_of(i) in LARGE_MESHES) == large)]

    def ordinary(self):
        """instances a record may be placed against: finite, not flat, of ordinary world size and seen by some cull mask"""
        skip = {"void", "singular", "huge!", "tiny!"}
        return [i for i, f in enumerate(self.families) if not skip & set(f) and self.mask_of(i)]


# ---- meshes -----------------------------------------------------------------------------------------------------------------------------
def _torus():
    """640 triangles on a torus of radii 1 and 0.27, rows staggered by half a cell: aspects 0.68 .. 0.72 in object space"""
    R, r = 1.0, 0.27
    j, i = np.meshgrid(np.arange(TORUS_V), np.arange(TORUS_U), indexing="ij")
    u = 2 * np.pi * (i + 0.5 * (j % 2)) / TORUS_U
    v = 2 * np.pi * j / TORUS_V
    pos = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=-1).reshape(-1, 3)
    nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], axis=-1).reshape(-1, 3)
    tri = []
    for jj in range(TORUS_V):
        for ii in range(TORUS_U):
            a, b = jj * TORUS_U + ii, jj * TORUS_U + (ii + 1) % TORUS_U
            jn = (jj + 1) % TORUS_V
            c, d = jn * TORUS_U + ii, jn * TORUS_U + (ii + 1) % TORUS_U
            if jj % 2 == 0:       # the next row is shifted by +half a cell: c sits between a and b
                tri += [(a, b, c), (b, d, c)]
            else:                 # the next row is shifted by -half a cell: d sits between a and b
                tri += [(a, d, c), (a, b, d)]
    return pos, nrm, np.array(tri, np.uint32)


def _soup(rng):
    """12 to 40 triangles of aspect 0.5 and more in the unit cube, both windings"""
    n = int(rng.integers(12, 41))
    pos = []
    for _ in range(n):
        a = rng.uniform(-0.8, 0.8, 3)
        d = cc._unit(rng.normal(size=3)); e = cc._unit(np.cross(d, rng.normal(size=3)))
        s = rng.uniform(0.15, 0.5)
        pos += [a, a + s * d, a + s * (rng.uniform(0.3, 0.7) * d + rng.uniform(0.7, 1.0) * e)]
    pos = np.array(pos)
    return pos, cc._unit(rng.normal(size=3)) * np.ones_like(pos), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def geometry(rng):
    """(verts, idx, ranges, object-space centre and radius per mesh, the far offset): the cube and octahedron of cull_cases, a soup, the
    torus, the torus moved 1000 to 10 000 away from the object-space origin, the torus scaled by 1e3 and by 1e-3, the soup moved away"""
    from vulkan_raytracing_amd import host
    paths = cc.mesh_paths()
    g = host.SceneGeometry([paths[cc.CUBE], paths[cc.OCTA]])
    verts, idx, ranges = [np.asarray(g.verts, np.float32).reshape(-1, 6)], [np.asarray(g.idx, np.uint32)], list(g.ranges)

    def add(pos, nrm, tri):
        ranges.append((6 * sum(len(v) for v in verts), sum(len(i) for i in idx), len(tri)))
        verts.append(np.concatenate([pos, nrm], axis=1).astype(np.float32)); idx.append(np.asarray(tri, np.uint32).reshape(-1))

    sp, sn, st = _soup(rng)
    tp, tn, tt = _torus()
    far = np.round(rng.uniform(1000.0, 10000.0, 3) * rng.choice([-1.0, 1.0], 3))
    add(sp, sn, st); add(tp, tn, tt); add(tp + far, tn, tt); add(tp * 1.0e3, tn, tt); add(tp * 1.0e-3, tn, tt); add(sp + far, sn, st)
    centre = np.array([(0, 0, 0)] * 4 + [far, (0, 0, 0), (0, 0, 0), far], np.float64)
    radius = np.array([1.0, 1.0, 1.0, 1.27, 1.27, 1.27e3, 1.27e-3, 1.0])
    return np.concatenate(verts).reshape(-1), np.concatenate(idx), ranges, centre, radius, far


def mesh_triangles(verts, idx, ranges, mesh):
    """(prims, 3, 3) binary64 object-space vertices of a mesh"""
    ff, fi, pc = ranges[mesh]
    p = np.asarray(verts, np.float32)[ff:].reshape(-1, 6)[:, :3].astype(np.float64)
    return p[np.asarray(idx[fi:fi + 3 * pc], np.int64).reshape(-1, 3)]


def aspects(T):
    """2 area / longest_edge^2 of (n, 3, 3) triangles, binary64 (0 for a zero-area triangle)"""
    e = np.stack([T[:, 1] - T[:, 0], T[:, 2] - T[:, 1], T[:, 0] - T[:, 2]], axis=1)
    longest2 = (e * e).sum(-1).max(axis=1)
    area2 = np.linalg.norm(np.cross(e[:, 0], -e[:, 2]), axis=1)
    return area2 / np.where(longest2 > 0, longest2, 1.0)


def world_triangles(scene, i):
    """(prims, 3, 3) binary64 world vertices of instance i (its binary32 record over the binary32 vertices)"""
    M = cc.matrix(scene.instances[i])
    return mesh_triangles(scene.verts, scene.idx, scene.ranges, scene.mesh_of(i)) @ M[:, :3].T + M[:, 3]


def condition(record):
    L = cc.matrix(record)[:, :3]
    if not np.isfinite(L).all():
        return np.nan
    s = np.linalg.svd(L, compute_uv=False)
    return s[0] / s[2] if s[2] > 0 else np.inf


# ---- instances ------------------------------------------------------------------------------------------------------------------------
def _linear(rng, family, cond):
    """a 3x3 matrix of the family with the largest singular value 1"""
    if family == "anisotropic" or family == "cancelling":
        s = np.array([1.0, cond ** -rng.uniform(0.0, 1.0), 1.0 / cond])
        return cc._rot(rng.normal(size=3), rng.uniform(0.3, 3.0)) @ np.diag(s) @ cc._rot(rng.normal(size=3), rng.uniform(0.3, 3.0)).T
    if family == "sheared":
        # unit columns, the third nearly in the plane of the other two: x -> x + k z, y -> y + k z and z scaled, rotated
        k = rng.uniform(0.6, 0.8) * rng.choice([-1.0, 1.0], 2)
        S = np.array([[1.0, 0.0, k[0]], [0.0, 1.0, k[1]], [0.0, 0.0, 1.0]])
        lo, hi = 0.0, 1.0      # bisection on the third column's height for sigma_min / sigma_max = 1 / cond
        for _ in range(60):
            S[2, 2] = 0.5 * (lo + hi)
            sv = np.linalg.svd(S, compute_uv=False)
            lo, hi = (S[2, 2], hi) if sv[2] / sv[0] < 1.0 / cond else (lo, S[2, 2])
        S = cc._rot(rng.normal(size=3), rng.uniform(0.3, 3.0)) @ S
        return S / np.linalg.svd(S, compute_uv=False)[0]
    raise ValueError(family)


def _dyadic(x, q=0.25):
    return np.round(np.asarray(x, np.float64) / q) * q


def _instances(rng, index, verts, idx, ranges, centre, radius):
    from vulkan_raytracing_amd.api import INSTANCE_DTYPE
    recs, fams, metas = [], [], []
    cells = [np.array([x, y, z], np.float64) * 4.0 for z in (0, 1) for y in (-1, 0, 1) for x in (-1, 0, 1)]
    order = rng.permutation(len(cells))
    hosts = []       # (centre, half extent) of the rigid_dyadic instances: where the nested ones go

    def tris(mesh):
        return mesh_triangles(verts, idx, ranges, mesh)

    def put(L, at, mesh, fam, meta):
        k = len(recs)
        t = np.asarray(at, np.float64) - L @ centre[mesh]
        r = cc._record(L, t, k, mesh, mask=1 << (k % 8))
        recs.append(r); fams.append(fam); metas.append(meta)
        return k

    slot = 0
    for family, mesh, par in _PLAN[index]:
        mirrored = isinstance(par, str) and par.endswith("m")
        ordinary = par == "o"
        target = int(str(par).rstrip("mo") or 0)
        at = cells[order[slot]] + rng.uniform(-0.5, 0.5, 3); slot += 1
        size = rng.uniform(1.2, 1.8)          # the world radius aimed at
        meta, tags = {}, [family]
        if family == "rigid_dyadic":
            s = float(rng.choice([0.5, 1.0, 1.5]))
            L = np.eye(3) * s
            at = _dyadic(at)
            hosts.append((at, s * radius[mesh] * (0.2 if mesh in LARGE_MESHES else 0.25)))
        elif family in ("anisotropic", "sheared", "cancelling"):
            cond = float(target or 1000)
            for attempt in range(8):         # the aspect floor: halve the condition number until every world triangle keeps it
                sub = np.random.default_rng([int(rng.integers(1 << 30)), attempt])
                L = _linear(sub, family, cond) * size / radius[mesh]
                L32 = L.astype(np.float32).astype(np.float64)
                if aspects(tris(mesh) @ L32.T).min() >= 1.05 * ASPECT_FLOOR:
                    break
                cond *= 0.5
            else:
                raise AssertionError("no draw of %s at the aspect floor" % family)
            meta.update(target=float(target or 1000), condition=cond, halved=attempt)
        elif family in ("tiny", "huge"):
            s = 1.0e-3 if family == "tiny" else 1.0e3
            L = cc._rot(rng.normal(size=3), rng.uniform(0.3, 3.0)) * s
            meta.update(scale=s, ordinary=ordinary)
            if not ordinary:
                tags.append(family + "!")
                if family == "huge":
                    at = np.zeros(3)           # (an octahedron or cube two thousand across around the whole scene)
        elif family == "coincident":
            L = cc._rot(rng.normal(size=3), rng.uniform(0.3, 3.0)) @ np.diag(rng.uniform(0.7, 1.3, 3)) * size / radius[mesh]
        elif family == "nested":
            c, h = hosts[0]
            L = np.eye(3) * _dyadic(h / radius[mesh], 2.0 ** -6)
            at = c
            meta.update(host=[i for i, f in enumerate(fams) if f[0] == "rigid_dyadic"][0])
        elif family == "singular":
            L = cc._rot(rng.normal(size=3), rng.uniform(0.3, 3.0)) @ np.diag([1.0, rng.uniform(0.5, 1.0), 0.0]) * size / radius[mesh]
        elif family == "void":
            L = cc._rot(rng.normal(size=3), rng.uniform(0.3, 3.0)) * size / radius[mesh]
        else:
            raise ValueError(family)
        if mirrored:
            L = L @ np.diag([-1.0, 1.0, 1.0]); tags.append("mirrored")
        k = put(L, at, mesh, tuple(tags), meta)
        if family == "void":
            recs[k]["transform"][int(rng.integers(0, 12))] = np.nan
        if family == "coincident":          # the same record again, not next to the first in the array
            meta["twin"] = None
    # the twins of the coincident instances go behind everything else, the enclosing cube last
    for k in [i for i, f in enumerate(fams) if f[0] == "coincident"]:
        r = recs[k].copy()
        j = len(recs)
        recs.append(r); fams.append(fams[k]); metas.append(dict(twin=k)); metas[k]["twin"] = j
    P = np.concatenate([world for world in (_world_points(recs[i], tris(int(recs[i]["mesh"]))) for i in range(len(recs))
                                               if "huge!" not in fams[i] and "void" not in fams[i])])
    lo, hi = P.min(0), P.max(0)
    recs.append(cc._record(np.diag(0.5 * (hi - lo) + 1.0), 0.5 * (lo + hi), len(recs), CUBE, mask=0))
    fams.append(("masked",)); metas.append({})
    fams = [f if f[0] in ("masked", "void") else f + ("masked",) for f in fams]      # (every other instance has one distinct mask bit)
    inst = np.asarray(recs, INSTANCE_DTYPE)
    for k in range(len(inst)):              # instance flags: every combination of the four bits somewhere in the set
        j = min(k, metas[k].get("twin", k))     # (a coincident pair is one record twice)
        inst[k]["sbt_offset_and_flags"] = (int(inst[k]["sbt_offset_and_flags"]) & 0x00FFFFFF) | (((5 * j + index) % 16) << 24)
    return inst, fams, metas


def _world_points(record, T):
    M = cc.matrix(record)
    return (T @ M[:, :3].T + M[:, 3]).reshape(-1, 3)


def scenes(seed=DEFAULT_SEED, n=N_SCENES):
    for index in range(n):
        rng = np.random.default_rng([seed, index])
        verts, idx, ranges, centre, radius, far = geometry(rng)
        inst, fams, metas = _instances(rng, index, verts, idx, ranges, centre, radius)
        shift = SCENE_SHIFT.get(index, 0.0)
        if shift:
            T = inst["transform"].astype(np.float64)
            T[:, [3, 7, 11]] += shift
            inst["transform"] = T.astype(np.float32)
        sc = Scene(index, seed, verts, idx, ranges, inst, fams, metas, shift)
        sc.far = far
        yield sc


# ---- query records ------------------------------------------------------------------------------------------------------------------------
class Placement:
    """what the record generators place against: per ordinary instance its binary64 world triangles, and the scene's box over them"""

    def __init__(self, scene):
        self.scene = scene
        self.inst = scene.ordinary()
        self.T = {i: world_triangles(scene, i) for i in self.inst}
        P = np.concatenate([t.reshape(-1, 3) for t in self.T.values()])
        self.lo, self.hi = P.min(0), P.max(0)
        self.c, self.diag = 0.5 * (self.lo + self.hi), float(np.linalg.norm(self.hi - self.lo))
        self.size = {i: float(np.linalg.norm(t.reshape(-1, 3).max(0) - t.reshape(-1, 3).min(0))) for i, t in self.T.items()}
        # the instance's own scale: the edge length of its median world triangle (a flattened instance is thin: distances count in this)
        self.scale = {i: float(np.median(np.linalg.norm(t[:, 1] - t[:, 0], axis=1))) for i, t in self.T.items()}

    def targets(self, n):
        """n instance indices, round robin over the ordinary instances"""
        return np.array([self.inst[k % len(self.inst)] for k in range(n)])

    def surface(self, rng, tgt):
        """(points, unit normals, triangle vertices): uniform barycentric samples of random triangles of the target instances"""
        q, nrm, tri = np.zeros((len(tgt), 3)), np.zeros((len(tgt), 3)), np.zeros((len(tgt), 3, 3))
        for j, i in enumerate(tgt):
            t = self.T[i][rng.integers(0, len(self.T[i]))]
            w = rng.dirichlet((1.0, 1.0, 1.0))
            q[j] = w @ t
            nrm[j] = cc._unit(np.cross(t[1] - t[0], t[2] - t[0]))
            tri[j] = t
        return q, nrm, tri

    def box_of(self, i):
        P = self.T[i].reshape(-1, 3)
        return P.min(0), P.max(0)


def _units(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _corner_points(pl, rng, tgt, lo_f=0.02, hi_f=0.12):
    """inside the world box of the target and near a corner of it (outside the mesh for the meshes here: none fills its box's corners)"""
    out = np.zeros((len(tgt), 3))
    for j, i in enumerate(tgt):
        lo, hi = pl.box_of(i)
        side = rng.integers(0, 2, 3)
        f = rng.uniform(lo_f, hi_f, 3)
        out[j] = np.where(side, hi - f * (hi - lo), lo + f * (hi - lo))
    return out


def _equidistant_points(pl, rng, n):
    """centres of the dyadic cubes and octahedra (every face at the same exact distance), midpoints between the centres of a coincident
    pair's two copies (the same place: every answer ties between the copies), points on the mirror plane of the dyadic instances"""
    sc = pl.scene
    out = []
    dy = [i for i in sc.with_family("rigid_dyadic") if i in pl.T]
    co = [i for i in sc.with_family("coincident") if i in pl.T]
    for k in range(n):
        pick = k % 3
        if pick == 0 or not co:
            i = dy[k % len(dy)]
            c = cc.matrix(sc.instances[i])[:, 3]
            s = abs(cc.matrix(sc.instances[i])[1, 1])
            # the centre, or the centre moved along an axis by a dyadic step: still equidistant from four faces of a cube / octahedron
            step = np.zeros(3); step[(k // 3) % 3] = (0.0, 0.125, -0.25, 0.5)[(k // 9) % 4] * s
            out.append(_f32(c + step))
        elif pick == 1:
            i = co[k % len(co)]
            q, _, _ = pl.surface(rng, [i])
            out.append(q[0] + _units(rng, 1)[0] * pl.scale[i] * 10 ** rng.uniform(-3, 0))
        else:
            i = dy[k % len(dy)]
            lo, hi = pl.box_of(i)
            p = rng.uniform(lo - 0.5, hi + 0.5)
            a = 2 if sc.mesh_of(i) in LARGE_MESHES else (k // 3) % 3
            p[a] = 0.5 * (lo[a] + hi[a])            # on a symmetry plane of the dyadic mesh (cube, octahedron; the torus in z)
            out.append(_f32(p))
    return np.array(out)


def point_records(scene, seed=DEFAULT_SEED, n=N_RECORDS):
    """{family: ((n, 4) float32 records with r_max = inf, the instance each was placed against or -1)}"""
    rng = np.random.default_rng([seed, scene.index, 1])
    pl = Placement(scene)
    tgt = pl.targets(n)
    out = {}
    q, nrm, _ = pl.surface(rng, tgt)
    off = np.array([pl.scale[i] for i in tgt]) * 10 ** rng.uniform(-4, -1, n) * rng.choice([-1.0, 1.0], n)
    out["near_surface"] = (q + nrm * off[:, None], tgt)
    feat = np.zeros((n, 3))
    for j, i in enumerate(tgt):
        t = pl.T[i][rng.integers(0, len(pl.T[i]))]
        feat[j] = t[j % 3] if j % 2 == 0 else t[0] + rng.uniform() * (t[1] - t[0])
    out["on_feature"] = (feat, tgt)
    out["volume"] = (pl.c + rng.uniform(-0.55, 0.55, (n, 3)) * (pl.hi - pl.lo), np.full(n, -1))
    out["far"] = (pl.c + _units(rng, n) * 50.0 * pl.diag, np.full(n, -1))
    out["box_corner"] = (_corner_points(pl, rng, tgt), tgt)
    out["equidistant"] = (_equidistant_points(pl, rng, n), np.full(n, -1))
    return {k: (np.concatenate([p, np.full((n, 1), np.inf)], axis=1).astype(np.float32), np.asarray(t)) for k, (p, t) in out.items()}


def radius_at_answer(records, t, column=3):
    """the records three times over with r_max (word `column`) set to the reference's t, to nextafter below it and above it (hits of the
    reference only: a miss keeps an infinite radius)"""
    t = np.asarray(t, np.float32)
    ok = np.isfinite(t)
    base = np.asarray(records, np.float32)[ok]
    out = []
    for r in (t[ok], np.nextafter(t[ok], np.float32(-np.inf)), np.nextafter(t[ok], np.float32(np.inf))):
        q = base.copy(); q[:, column] = np.maximum(r, np.float32(0.0))
        out.append(q)
    return np.concatenate(out)


def sweep_records(scene, seed=DEFAULT_SEED, n=N_RECORDS):
    """{family: ((n, 8) float32 sweeps (o, r, d, tmax), target)}: aimed, grazing at r (1 +- 1e-3), axis-parallel directions, starting
    inside, short and long tmax around the contact, radii of 1e-3 and of 10 instance sizes and 0, d scaled by 1e-3 and 1e3"""
    rng = np.random.default_rng([seed, scene.index, 2])
    pl = Placement(scene)
    tgt = pl.targets(n)
    size = np.array([pl.size[i] for i in tgt]); scale = np.array([pl.scale[i] for i in tgt])

    def pack(o, r, d, tmax):
        s = np.zeros((len(o), 8)); s[:, 0:3] = o; s[:, 3] = r; s[:, 4:7] = d; s[:, 7] = tmax
        return s.astype(np.float32)

    out = {}
    q, nrm, _ = pl.surface(rng, tgt)
    d = _units(rng, n)
    dist = size * rng.uniform(1.0, 3.0, n)
    r = scale * 10 ** rng.uniform(-2, 0, n)
    out["aimed"] = pack(q - d * dist[:, None], r, d, np.inf)
    # grazing: past an edge point at r (1 +- 1e-3), perpendicular to the edge and to d
    _, _, tri = pl.surface(rng, tgt)
    e = tri[:, 1] - tri[:, 0]
    P = tri[:, 0] + rng.uniform(size=(n, 1)) * e
    d = _units(rng, n)
    w = np.cross(d, e); w /= np.linalg.norm(w, axis=1, keepdims=True)
    r = scale * 10 ** rng.uniform(-2, 0, n)
    off = r * (1 + 1e-3 * rng.choice([-1.0, 1.0], n))
    out["grazing"] = pack(P + w * off[:, None] - d * dist[:, None], r, d, np.inf)
    d = np.zeros((n, 3))
    k = np.arange(n)
    d[k, k % 3] = rng.choice([-1.0, 1.0], n)
    two = (k % 2 == 1)
    d[k[two], (k[two] + 1) % 3] = rng.uniform(-1, 1, two.sum())           # one exact zero component; the others have two
    out["axis_parallel"] = pack(_f32(q) - d * dist[:, None], scale * 10 ** rng.uniform(-2, 0, n), d, np.inf)
    r = scale * 10 ** rng.uniform(-1.5, 0.5, n)
    out["inside"] = pack(q + _units(rng, n) * (r * rng.uniform(0, 1, n))[:, None], r, _units(rng, n), size * rng.uniform(0.1, 2.0, n))
    d = _units(rng, n)
    r = scale * 10 ** rng.uniform(-2, 0, n)
    tm = np.where(k % 3 == 0, np.inf, np.where(k % 3 == 1, (dist - r) * (1 - 1e-3), (dist - r) * (1 + 1e-3)))
    out["tmax"] = pack(q - d * dist[:, None], r, d, np.maximum(tm, 0.0))
    d = _units(rng, n)
    r = np.where(k % 3 == 0, 1e-3 * size, np.where(k % 3 == 1, 10.0 * size, 0.0))
    start = np.where((k % 3 == 1)[:, None], q - d * (dist + 25.0 * size)[:, None], q - d * dist[:, None])
    out["radii"] = pack(start, r, d, np.inf)
    d = _units(rng, n)
    ln = np.where(k % 2 == 0, 1e-3, 1e3)
    out["scaled_d"] = pack(q - d * dist[:, None], scale * 10 ** rng.uniform(-2, 0, n), d * ln[:, None], np.where(k % 4 < 2, np.inf, 2 * dist / ln))
    return {name: (s, tgt) for name, s in out.items()}


def box_records(scene, seed=DEFAULT_SEED, n=N_RECORDS):
    """{family: ((n, 8) float32 boxes (lo, ignored, hi, ignored), target)}: a face coplanar with a face of a dyadic instance, lo == hi
    on one, two and three axes, tiny boxes, the enclosing box, boxes in the corners of an instance's world box"""
    rng = np.random.default_rng([seed, scene.index, 3])
    pl = Placement(scene)
    tgt = pl.targets(n)
    scale = np.array([pl.scale[i] for i in tgt])

    def pack(lo, hi):
        b = np.zeros((len(lo), 8), np.float32)
        b[:, 0:3] = lo; b[:, 4:7] = hi; b[:, 3] = 7.0; b[:, 7] = np.nan
        return b

    out = {}
    dy = [i for i in scene.with_family("rigid_dyadic") if i in pl.T]
    lo, hi = np.zeros((n, 3)), np.zeros((n, 3))
    for j in range(n):
        i = dy[j % len(dy)]
        blo, bhi = pl.box_of(i)
        a, side = j % 3, (j // 3) % 2
        c = _f32(rng.uniform(blo, bhi)); h = rng.uniform(0.05, 0.6, 3) * (bhi - blo)
        if j % 2 == 0:                    # over the middle of the face: the octahedron's apex, the torus's flat ring
            c = _f32(0.5 * (blo + bhi) + rng.uniform(-0.2, 0.2, 3) * (bhi - blo)); h = rng.uniform(0.3, 0.6, 3) * (bhi - blo)
        lo[j], hi[j] = c - h, c + h
        if side:                          # the box's low face on the instance's high plane, or its high face on the low plane
            lo[j, a] = bhi[a]; hi[j, a] = bhi[a] + h[a]
        else:
            hi[j, a] = blo[a]; lo[j, a] = blo[a] - h[a]
    out["coplanar_face"] = (pack(lo, hi), np.array([dy[j % len(dy)] for j in range(n)]))
    q, _, tri = pl.surface(rng, tgt)
    q = np.where((np.arange(n) % 4 == 3)[:, None], tri[:, 0], q)              # (every fourth on a vertex)
    q32 = _f32(q)
    h = scale[:, None] * 10 ** rng.uniform(-1.5, 0.5, (n, 3))
    lo, hi = q32 - h, q32 + h
    axes = np.array([(1, 2, 4, 3, 5, 6, 7)[j % 7] for j in range(n)])
    for a in range(3):
        m = (axes >> a) & 1 == 1
        lo[m, a] = q32[m, a]; hi[m, a] = q32[m, a]
    out["collapsed"] = (pack(lo, hi), tgt)
    mag = np.abs(q).max(axis=1)
    h = np.maximum(scale * 10 ** rng.uniform(-3, -1, n), 2.0 ** -14 * mag)[:, None] * rng.uniform(0.3, 1.0, (n, 3))
    q2 = q + _units(rng, n) * h
    tiny = pack(q2 - h, q2 + h)
    tiny[-1] = pack((pl.lo - 1.0)[None], (pl.hi + 1.0)[None])[0]                 # the box around the whole scene
    out["tiny_and_enclosing"] = (tiny, tgt)
    c = _corner_points(pl, rng, tgt, 0.03, 0.1)
    h = np.array([pl.box_of(i)[1] - pl.box_of(i)[0] for i in tgt]) * 10 ** rng.uniform(-2, -0.5, (n, 1)) * rng.uniform(0.3, 1.0, (n, 3))
    out["box_corner"] = (pack(c - h, c + h), tgt)
    size = (pl.hi - pl.lo).max() * 10 ** rng.uniform(-2, -0.5, (n, 1)) * rng.uniform(0.3, 1.0, (n, 3))
    ctr = q + rng.uniform(-1.0, 1.0, (n, 3)) * size                                  # (boxes of every size about the surface)
    out["volume"] = (pack(ctr - size / 2, ctr + size / 2), tgt)
    return out


def segment_records(scene, seed=DEFAULT_SEED, n=N_RECORDS):
    """{family: ((n, 8) float32 capsule records (p0, r_max, p1, ignored), target)}: crossing a surface, nearly parallel to a face at
    1e-3 of its size, spanning the whole scene, tiny, and a point; r_max = inf"""
    rng = np.random.default_rng([seed, scene.index, 4])
    pl = Placement(scene)
    tgt = pl.targets(n)
    scale = np.array([pl.scale[i] for i in tgt])[:, None]

    def pack(p0, p1):
        s = np.zeros((len(p0), 8)); s[:, 0:3] = p0; s[:, 3] = np.inf; s[:, 4:7] = p1
        return s.astype(np.float32)

    out = {}
    q, nrm, tri = pl.surface(rng, tgt)
    d = _units(rng, n)
    out["crossing"] = (pack(q - d * scale * rng.uniform(0.1, 2.0, (n, 1)), q + d * scale * rng.uniform(0.1, 2.0, (n, 1))), tgt)
    e = tri[:, 1] - tri[:, 0]; f = tri[:, 2] - tri[:, 0]
    size = np.linalg.norm(e, axis=1, keepdims=True)
    a0, a1 = q + nrm * 1e-3 * size, q + rng.uniform(-1, 1, (n, 1)) * e + rng.uniform(-1, 1, (n, 1)) * f + nrm * 1e-3 * size * rng.uniform(0.9, 1.1, (n, 1))
    out["nearly_parallel"] = (pack(a0, a1), tgt)
    p0 = pl.c + rng.uniform(-0.7, 0.7, (n, 3)) * (pl.hi - pl.lo)
    out["spanning"] = (pack(p0, q + rng.uniform(0.1, 0.5, (n, 1)) * (q - p0)), tgt)            # (through a surface point and on)
    p = q + _units(rng, n) * scale * 10 ** rng.uniform(-3, 0, (n, 1))
    mag = np.abs(p).max(axis=1, keepdims=True)
    out["tiny"] = (pack(p, p + _units(rng, n) * np.maximum(scale * 10 ** rng.uniform(-4, -2, (n, 1)), 2.0 ** -18 * mag)), tgt)
    out["point"] = (pack(p, p), tgt)
    return out


def triangle_records(scene, seed=DEFAULT_SEED, n=N_RECORDS):
    """{family: ((n, 12) float32 triangle records (P0, r_max, P1, ignored, P2, ignored), target)}: crossing a surface, nearly parallel
    to a face at 1e-3 of its size, spanning the scene, tiny, and the degenerate forms (a point, a segment); r_max = inf.  The same
    records serve rt_overlap_triangles_device, where word 3 is ignored."""
    rng = np.random.default_rng([seed, scene.index, 5])
    pl = Placement(scene)
    tgt = pl.targets(n)
    scale = np.array([pl.scale[i] for i in tgt])[:, None]

    def pack(p0, p1, p2):
        s = np.zeros((len(p0), 12)); s[:, 0:3] = p0; s[:, 3] = np.inf; s[:, 4:7] = p1; s[:, 8:11] = p2
        return s.astype(np.float32)

    out = {}
    q, nrm, tri = pl.surface(rng, tgt)
    d, e = _units(rng, n), _units(rng, n)
    w = scale * rng.uniform(0.2, 2.0, (n, 1))
    out["crossing"] = (pack(q - d * w, q + d * w + e * w * 0.3, q + d * w - e * w * 0.5), tgt)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    size = np.linalg.norm(e1, axis=1, keepdims=True)
    h = nrm * 1e-3 * size
    uv = rng.uniform(-0.5, 1.5, (3, 2, n, 1))
    uv[0] = rng.uniform(0.2, 0.4, (2, n, 1))
    # (every second record with its first vertex below the face and the others above: it cuts the face at a slope of about 1e-3)
    sg = [np.where((np.arange(n) % 2 == 1)[:, None], -1.0, 1.0), 1.0, 1.0]
    out["nearly_parallel"] = (pack(*(tri[:, 0] + uv[j, 0] * e1 + uv[j, 1] * e2 + sg[j] * h * rng.uniform(0.9, 1.1, (n, 1)) for j in range(3))), tgt)
    p0, p1 = (pl.c + rng.uniform(-0.7, 0.7, (n, 3)) * (pl.hi - pl.lo) for _ in range(2))
    out["spanning"] = (pack(p0, p1, q + rng.uniform(0.1, 0.5, (n, 1)) * (q - p0)), tgt)          # (an edge through a surface point and on)
    mag = np.abs(q).max(axis=1, keepdims=True)
    s = np.maximum(scale * 10 ** rng.uniform(-4, -2, (n, 1)), 2.0 ** -16 * mag)
    p = q + _units(rng, n) * s * rng.uniform(0.0, 0.8, (n, 1))                                    # (about half of them reach the surface)
    out["tiny"] = (pack(p, p + _units(rng, n) * s, p + _units(rng, n) * s), tgt)
    d = _units(rng, n)
    w = scale * rng.uniform(0.05, 1.0, (n, 1))
    k = (np.arange(n) % 2 == 0)[:, None]
    on = _f32(np.where((np.arange(n) % 4 == 0)[:, None], tri[:, 0], q))                           # a point: on a vertex, or on a face to rounding
    out["degenerate"] = (pack(np.where(k, on, q - d * w), np.where(k, on, q + d * w), np.where(k, on, q + d * w)), tgt)   # a point; a segment (P1 == P2)
    return out


# ---- a scene with its records and brute-force references, computed once and shared by the CPU and the GPU test files ----------------
QUERIES = ("closest_point", "closest_point_hits", "point_inside", "overlap_boxes", "overlap_triangles", "sweep_spheres", "closest_segment",
           "closest_triangle")
MAX_ROWS = 16                  # the references of the list forms are taken at 16 rows and truncated
CULL_STRIDE = {"closest_segment": 4, "closest_triangle": 4}      # cull masks other than 0xFF run on every fourth record of these
RADIUS_STRIDE = {"closest_point": 4, "closest_point_hits": 4, "closest_segment": 4, "closest_triangle": 8}


class World:
    """one scene, closest_reference.Scene over it, per query the records (every family behind one another, then radius_at_answer from
    the reference's own t where the query has a radius, then the invalid records of the query's own test file) with the family and the
    target instance of every record, and reference(query, cull): the brute force of that query's reference module, cached"""

    def __init__(self, scene, seed=DEFAULT_SEED):
        from tests import closest_reference as cr, overlap_reference as orf
        self.scene, self.seed = scene, seed
        self.S = cr.Scene(*scene.parts)
        self.tris = orf.Triangles(self.S)
        self._sets, self._refs, self.seconds = {}, {}, {}
        self.n_tris = np.array([scene.ranges[scene.mesh_of(i)][2] for i in range(len(scene.instances))], np.int64)

    def admitted_triangles(self, cull):
        """the triangles a walk can reach under the cull mask (a void record has no image and no box: the walks never enter it)"""
        return int(sum(self.n_tris[i] for i in range(len(self.n_tris)) if self.scene.mask_of(i) & cull and "void" not in self.scene.families[i]))

    def culls(self, query):
        """0xFF, one bit (that of the instance the reference names most often), and 0xFF without that bit: the nearest instance left out"""
        ref = self.reference(query, 0xFF)
        h = ref[0] if isinstance(ref, tuple) else ref
        if query in ("overlap_boxes", "overlap_triangles"):
            named = ref[1][..., 0][ref[1][..., 0] >= 0]
        elif query == "point_inside":
            return (0xFF, 1 << (self.scene.index % 8), 0xFF & ~(1 << (self.scene.index % 8)))
        else:
            named = h["inst"][h["inst"] >= 0]
        bit = self.scene.mask_of(int(np.bincount(named.reshape(-1)).argmax())) if len(named) else 1
        return (0xFF, bit, 0xFF & ~bit)

    def _base(self, query):
        sc = self.scene
        if query in ("closest_point", "closest_point_hits", "point_inside"):
            return point_records(sc, self.seed)
        if query == "overlap_boxes":
            return box_records(sc, self.seed)
        if query == "sweep_spheres":
            return sweep_records(sc, self.seed)
        if query == "closest_segment":
            return segment_records(sc, self.seed)
        return triangle_records(sc, self.seed)

    def records(self, query):
        """(records, family name per record (an array of str), target instance per record or -1)"""
        if query in self._sets:
            return self._sets[query]
        base = self._base(query)
        recs = [r for r, _ in base.values()]
        fam = [np.full(len(r), name) for name, (r, _) in base.items()]
        tgt = [np.asarray(t, np.int64) for _, t in base.values()]
        if query in RADIUS_STRIDE:
            key = "closest_point" if query == "closest_point_hits" else query
            if key != query:
                extra = self.records(key)
                extra = extra[0][extra[1] == "radius_at_answer"]
            else:
                self._sets[query] = (np.concatenate(recs), np.concatenate(fam), np.concatenate(tgt))
                ref = self._compute(query, 0xFF)
                h = ref[0] if isinstance(ref, tuple) else ref
                pick = np.arange(0, len(h), RADIUS_STRIDE[query])
                pick = pick[h["inst"][pick] >= 0]
                extra = radius_at_answer(self._sets[query][0][pick], h["t"][pick])
            recs.append(extra); fam.append(np.full(len(extra), "radius_at_answer")); tgt.append(np.full(len(extra), -1, np.int64))
        from tests import test_closest_point as tcp, test_closest_segment as tcs, test_closest_triangle as tct, test_overlap_boxes as tob
        from tests import test_sphere_sweep as tss, test_triangle_overlaps as tto
        first = recs[0]
        bad = {"closest_point": tcp.invalid_records, "closest_point_hits": tcp.invalid_records, "point_inside": tcp.invalid_records,
               "overlap_boxes": tob.invalid_boxes, "overlap_triangles": tto.invalid_tris, "sweep_spheres": tss.invalid_sweeps,
               "closest_segment": tcs.invalid_records, "closest_triangle": tct.invalid_records}[query](first)
        recs.append(np.asarray(bad, np.float32)); fam.append(np.full(len(bad), "invalid")); tgt.append(np.full(len(bad), -1, np.int64))
        self._sets[query] = (np.ascontiguousarray(np.concatenate(recs), np.float32), np.concatenate(fam), np.concatenate(tgt))
        return self._sets[query]

    def use_records(self, query, records, family, target=None):
        """records from outside in place of the generated ones (a subset of another World's, as they are)"""
        n = len(records)
        self._sets[query] = (np.ascontiguousarray(records, np.float32), np.asarray(family), np.full(n, -1, np.int64) if target is None else np.asarray(target))
        for key in [k for k in self._refs if k[0] == query]:
            del self._refs[key]

    def cached(self, key, make):
        """a reference of the caller's own (the oracle's counts and lists over this World's records), made once"""
        if ("extra", key) not in self._refs:
            self._refs[("extra", key)] = make()
        return self._refs[("extra", key)]

    def alone(self, i):
        """a World of instance i alone in the scene: the same geometry, one record"""
        sc = self.scene
        one = Scene(sc.index, sc.seed, sc.verts, sc.idx, sc.ranges, sc.instances[[i]], [sc.families[i]], [sc.meta[i]], sc.shift)
        one.name = "%s instance %d alone" % (sc.name, i)
        return World(one, self.seed)

    def overlap_cull(self, cull):
        """rt_api.h leaves pairs of two zero-area triangles open for rt_overlap_triangles_device: its zero-area records (the `degenerate`
        family) run with the singular instances' mask bits taken out of the cull mask"""
        for i in self.scene.with_family("singular"):
            cull &= ~self.scene.mask_of(i)
        return cull

    def _compute(self, query, cull, records=None):
        import time
        from tests import closest_hits_reference as chr_, closest_reference as cr, overlap_reference as orf, segment_reference as sgr
        from tests import sweep_reference as sr, triangle_distance_reference as tdr, triangle_overlap_reference as tor
        r = self._sets[query][0] if records is None else records
        t0 = time.perf_counter()
        if query == "closest_point" or query == "point_inside":
            out = cr.brute32(self.S, r, cull)
        elif query == "closest_point_hits":
            out = chr_.brute32_k(self.S, r, MAX_ROWS, cull)
        elif query == "overlap_boxes":
            out = orf.brute32(self.S, r, cull, MAX_ROWS, tris=self.tris)
        elif query == "overlap_triangles":
            out = tor.brute32(self.S, r, cull, MAX_ROWS, tris=self.tris)
        elif query == "sweep_spheres":
            out = sr.brute32(self.S, r, cull)
        elif query == "closest_segment":
            out = sgr.brute32(self.S, r, cull)
        elif query == "closest_triangle":
            out = tdr.brute32(self.S, r, cull)[:2]
        else:
            raise ValueError(query)
        self.seconds[query] = self.seconds.get(query, 0.0) + time.perf_counter() - t0
        return out

    def reference(self, query, cull=0xFF, stride=1):
        """the brute force over every stride-th record of the query (overlap_triangles: the degenerate family under overlap_cull(cull))"""
        if (query, cull, stride) not in self._refs:
            recs, fam, _ = self.records(query)
            recs, fam = recs[::stride], fam[::stride]
            out = self._compute(query, cull, recs)
            if query == "overlap_triangles":
                z = np.nonzero(fam == "degenerate")[0]
                part = self._compute(query, self.overlap_cull(cull), recs[z])
                for whole, piece in zip(out, part):
                    whole[z] = piece
            self._refs[(query, cull, stride)] = out
        return self._refs[(query, cull, stride)]


_WORLDS = {}


def world(index, seed=DEFAULT_SEED):
    """World of scene `index`, made once per process"""
    if (seed, index) not in _WORLDS:
        for sc in scenes(seed):
            if (seed, sc.index) not in _WORLDS:
                _WORLDS[(seed, sc.index)] = World(sc, seed)
    return _WORLDS[(seed, index)]
