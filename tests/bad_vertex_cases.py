"""Bad vertex positions (include/rt_api.h at rt_upload_geometry; DESIGN.md §5 "Bad vertices"): the case table, the meshes, the twin of a
mesh, the scene and the query records of tests/test_bad_vertices.py.  No GPU is needed here.

A triangle is BAD if one of its nine position coordinates is not finite or has magnitude >= 1e37; a bad triangle is inactive.  A case
is (coordinate class, pattern, mesh):
  class    what is written into a chosen vertex: NaN / +inf / -inf in y or in all three coordinates, +inf and -inf in two vertices of ONE
           triangle, 3e38, exactly 1e37 (BAD); the binary32 number just below 1e37, 1e30 (FAR: valid)
  pattern  which vertices are chosen: one, every 40th from 17, the first third, all, or one private vertex of a triangle that duplicates
           a good one
  mesh     the teapot, 9 / 8 / 7 random triangles, the degenerate soup, a bumpy grid above the host builder's threading threshold
Every mesh carries ONE extra vertex behind its own, all NaN, which no triangle of the mesh names.  The TWIN of a mesh is the same vertex
buffer with the three indices of every bad triangle pointed at that vertex: what the bad mesh has to equal, output buffer for output
buffer.  The twin is only ever given to the oracle and the references, never to the library."""
import os

import numpy as np

from tests import scenes
from tests import tree_reference as tr
from vulkan_raytracing_amd import host
from vulkan_raytracing_amd.api import INSTANCE_DTYPE

RES = scenes.RES
F = np.float32
LIMIT = F(1e37)
BELOW = np.nextafter(LIMIT, F(0))
N_RANDOM, N_AIMED, N_RECORDS = 20000, 4000, 512
FRAME_W, FRAME_H, SPP, BOUNCES = 64, 48, 2, 2


# ---- coordinate classes: f(pos (nv, 3) float32, chosen vertices, tri (nt, 3)) writes into pos ------------------------------------------

def _y(value):
    def f(pos, sel, tri):
        pos[sel, 1] = value
    return f


def _vertex(value):
    def f(pos, sel, tri):
        pos[sel] = value
    return f


def _inf_pm(pos, sel, tri):
    """+inf in y of the chosen vertex and -inf in y of the next vertex of the first triangle that names it: that triangle's box is
    (-inf, inf) on y and its centroid NaN"""
    for v in np.asarray(sel).tolist():
        t = tri[np.nonzero((tri == v).any(axis=1))[0][0]]
        other = [int(w) for w in t if int(w) != v][0]
        pos[v, 1] = np.inf
        pos[other, 1] = -np.inf


BAD = {"nan_y": _y(np.nan), "nan_vertex": _vertex(np.nan), "pinf_y": _y(np.inf), "ninf_y": _y(-np.inf), "pinf_vertex": _vertex(np.inf),
       "ninf_vertex": _vertex(-np.inf), "inf_pm": _inf_pm, "3e38_y": _y(F(3e38)), "1e37_y": _y(LIMIT)}
FAR = {"below_1e37_y": _y(BELOW), "1e30_y": _y(F(1e30))}
CLASSES = dict(BAD, **FAR)
NON_FINITE = ("nan_y", "nan_vertex", "pinf_y", "ninf_y", "pinf_vertex", "ninf_vertex", "inf_pm")

# ---- patterns: the chosen vertices of a mesh with nv vertices ---------------------------------------------------------------------------
PATTERNS = {"one": lambda nv: np.array([17]), "every40": lambda nv: np.arange(17, nv, 40), "first_third": lambda nv: np.arange(nv // 3),
            "all": lambda nv: np.arange(nv), "duplicate": None}

MESHES = ("teapot", "tri9", "tri8", "tri7", "soup")
_CACHE = {}


def clean(name):
    """(pos (nv, 3), normals (nv, 3), tri (nt, 3)) of a mesh of the table, float32 / int64"""
    if name not in _CACHE:
        from tests import test_tree_invariants as ti
        if name == "teapot":
            g = host.SceneGeometry([os.path.join(RES, "teapot.obj")])
            v, i = g.verts.reshape(-1, 6).copy(), g.idx.copy()
        elif name == "big":                                                       # 131 x 131 quads over a bumpy sheet: 34 322 triangles
            n = 131
            x, y = np.meshgrid(np.linspace(-3, 3, n + 1), np.linspace(-3, 3, n + 1), indexing="ij")
            pos = np.stack([x.ravel(), y.ravel(), 0.4 * np.sin(3 * x.ravel()) * np.cos(2 * y.ravel())], axis=1)
            a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
            v, i = ti._mesh(pos, np.stack([a, a + 1, a + n + 2, a, a + n + 2, a + n + 1], axis=1).reshape(-1, 3))
        else:
            v, i = ti.shapes()[name]
        v = np.asarray(v, F).reshape(-1, 6)
        _CACHE[name] = (v[:, :3].copy(), v[:, 3:].copy(), np.asarray(i, np.int64).reshape(-1, 3))
    return _CACHE[name]


def mesh(name, cls, pattern):
    """-> dict(verts (nv + 1, 6) float32 with the all-NaN vertex last, idx (3 nt,) uint32, bad (nt,) bool, touched (nt,) bool: the triangles
    that name a vertex the case wrote to, clean (nt, 3, 3): the positions before).  Pattern "duplicate" appends three private vertices
    with the positions of triangle nt // 2 and a triangle over them, and writes into the first of the three."""
    key = (name, cls, pattern)
    if key in _CACHE:
        return _CACHE[key]
    pos, nrm, tri = clean(name)
    pos, nrm, tri = pos.copy(), nrm.copy(), tri.copy()
    if pattern == "duplicate":
        src = tri[len(tri) // 2]
        sel = np.array([len(pos)])
        tri = np.concatenate([tri, [[len(pos), len(pos) + 1, len(pos) + 2]]])
        pos, nrm = np.concatenate([pos, pos[src]]), np.concatenate([nrm, nrm[src]])
    else:
        sel = PATTERNS[pattern](len(pos))
    pos0 = pos.copy()
    before = pos0[tri]
    CLASSES[cls](pos, sel, tri)
    written = np.nonzero((pos.view(np.uint32) != pos0.view(np.uint32)).any(axis=1))[0]
    verts = np.zeros((len(pos) + 1, 6), F)
    verts[:-1, :3], verts[:-1, 3:] = pos, nrm
    verts[-1] = np.nan
    out = dict(verts=verts, idx=tri.astype(np.uint32).reshape(-1), bad=~tr.active_triangles(pos[tri]), touched=np.isin(tri, written).any(axis=1), clean=before)
    _CACHE[key] = out
    return out


def twin_idx(m):
    """the index buffer of the twin: the bad triangles name the all-NaN vertex"""
    idx = m["idx"].reshape(-1, 3).copy()
    idx[m["bad"]] = len(m["verts"]) - 1
    return idx.reshape(-1)


# ---- the scene: two instances of the mesh (one rotated and sheared), a clean cube, one instance of an all-bad mesh -----------------------
# The scale 0.75 keeps the world box of a mesh with a coordinate just below 1e37 below the instance limit (rt_set_instances: a padded
# world box that reaches 1e37 makes its record void).
def _m(rows, t):
    return np.concatenate([np.asarray(rows, np.float64), np.asarray(t, np.float64)[:, None]], axis=1).astype(F).reshape(12)


_C, _S = np.cos(0.7), np.sin(0.7)
TRANSFORMS = [_m(np.eye(3) * 0.75, [0, -0.9, 0]),
              _m(0.6 * np.array([[_C, 0.3, _S], [0, 1, 0], [-_S, 0, _C]]), [5.0, -0.5, 1.0]),       # rotated about y, sheared (x += 0.3 y)
              _m(np.eye(3) * 0.8, [-4.0, 0.5, 0.5]),
              _m(np.eye(3) * 0.75, [0.0, 0.0, 4.0])]
INST_MESH = [0, 0, 1, 2]
INST_CUSTOM = [0, 0, 1, 0]


def instances(n=4):
    return np.array([host.make_instance(TRANSFORMS[i], INST_CUSTOM[i], INST_MESH[i]) for i in range(n)], INSTANCE_DTYPE)


def scene(name, cls, pattern):
    """-> dict(verts, idx, ranges: the three meshes as the library gets them; twin_idx: the twin's index buffer; uniforms; m: mesh 0).
    Mesh 2 is the teapot with the class written into ALL its vertices (for a far class: NaN into all, so that it is all bad)."""
    from tests import test_tree_invariants as ti
    key = ("scene", name, cls, pattern)
    if key in _CACHE:
        return _CACHE[key]
    m0 = mesh(name, cls, pattern)
    g = host.SceneGeometry([os.path.join(RES, "cube.obj")])
    m2 = mesh("teapot", cls if cls in BAD else "nan_vertex", "all")
    parts = [(m0["verts"], m0["idx"]), (g.verts.reshape(-1, 6), g.idx), (m2["verts"], m2["idx"])]
    verts, idx, ranges = ti.pack(parts)
    t_idx = np.concatenate([twin_idx(m0), g.idx, twin_idx(m2)])
    u = host.default_uniforms(max_bounce_count=BOUNCES, samples_per_pixel=SPP, center_object_type=1, orbiting_object_type=0,
                              orbiting_object_primitive_offset=ranges[1][1] // 3, orbiting_object_vertex_offset=ranges[1][0])
    out = dict(verts=verts, idx=idx, ranges=ranges, twin_idx=t_idx, uniforms=u, m=m0, name=name)
    _CACHE[key] = out
    return out


def oracle_scene(sc, twin, n_inst=4, clean_mesh=False):
    """an OracleScene over the scene's vertices as they are (twin False) or over the twin; clean_mesh: mesh 0 before the case wrote"""
    from oracle import oracle
    S = oracle.OracleScene()
    verts = sc["verts"]
    if clean_mesh:
        verts = verts.copy()
        v = verts[:sc["ranges"][1][0]].reshape(-1, 6)
        tri = sc["m"]["idx"].reshape(-1, 3).astype(np.int64)
        v[tri.reshape(-1), :3] = sc["m"]["clean"].reshape(-1, 3)
    S.set_geometry(verts, sc["twin_idx"] if twin and not clean_mesh else sc["idx"], sc["ranges"])
    inst = instances(n_inst)
    S.set_instances([inst[i].tobytes() for i in range(n_inst)])
    S.set_uniforms(sc["uniforms"].tobytes())
    S.set_skybox(scenes.synthetic_skybox(64))
    return S


def _world(M, p):
    M = np.asarray(M, np.float64).reshape(3, 4)
    return p @ M[:, :3].T + M[:, 3]


def surface_points(sc, n, seed, share_touched=0.5):
    """n world-space points on instance 0: random barycentric points of triangles of mesh 0 at their CLEAN positions, `share_touched` of
    them on the triangles the case wrote to"""
    rng = np.random.default_rng(seed)
    m = sc["m"]
    touched, others = np.nonzero(m["touched"])[0], np.nonzero(~m["touched"])[0]
    k = int(n * share_touched) if len(others) else n
    if not len(touched):
        k = 0
    t = np.concatenate([rng.choice(touched, k) if k else np.zeros(0, np.int64), rng.choice(others, n - k) if n - k else np.zeros(0, np.int64)]).astype(np.int64)
    b = rng.dirichlet([1, 1, 1], n)
    p = (m["clean"][t].astype(np.float64) * b[:, :, None]).sum(axis=1)
    return _world(TRANSFORMS[0], p)


def _aimed(sc, n, seed, share_touched):
    rng = np.random.default_rng(seed)
    tgt = surface_points(sc, n, seed + 1, share_touched)
    o = rng.normal(size=(n, 3)); o *= 12.0 / np.linalg.norm(o, axis=1, keepdims=True)
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = np.zeros((n, 8), F)
    out[:, 0:3] = o; out[:, 3] = 0.001; out[:, 4:7] = d; out[:, 7] = 10000.0
    return out


def rays(sc):
    """N_RANDOM rays followed by N_AIMED aimed ones (from a sphere of radius 12 at surface_points of instance 0, half of them on the
    triangles the case wrote to); tmin 0.001, tmax 10000.  The random ones: for the teapot scenes.random_rays(seed 5, origins within 12,
    targets within 1.5 of the origin: the issue's set, its target radius scaled as instance 0 is); the other meshes are too sparse for
    those to hit, theirs are aimed as well, one in ten at a triangle the case wrote to."""
    key = ("rays", id(sc))
    if key not in _CACHE:
        first = scenes.random_rays(N_RANDOM, seed=5, origin_radius=12.0, target_radius=1.5) if sc["name"] == "teapot" else _aimed(sc, N_RANDOM, 8, 0.1)
        _CACHE[key] = np.concatenate([first, _aimed(sc, N_AIMED, 6, 0.5)])
    return _CACHE[key]


def query_records(sc):
    """points (every fourth with radius 1, the others unbounded), sphere sweeps, boxes and query triangles about surface_points of
    instance 0 (three in ten on a triangle the case wrote to), in the record layouts of their generators (tests/instance_record_cases.py query_records)"""
    from tests.test_closest_point import with_radius
    from tests.test_overlap_boxes import as_boxes
    from tests.test_sphere_sweep import as_sweeps, unit
    key = ("records", id(sc))
    if key in _CACHE:
        return _CACHE[key]
    m = N_RECORDS
    rng = np.random.default_rng(11)
    near = lambda seed, r: surface_points(sc, m, seed, share_touched=0.3) + rng.uniform(-r, r, (m, 3))
    points = with_radius(near(12, 0.3), np.where(np.arange(m) % 4 == 0, 1.0, np.inf))
    o = unit(rng.normal(size=(m, 3))) * 12.0
    sweeps = as_sweeps(o, 10 ** rng.uniform(-2, -0.5, m), unit(near(13, 0.1) - o), np.where(np.arange(m) % 3 == 0, np.inf, 30.0))
    c = near(14, 0.1)
    h = 10 ** rng.uniform(-2, -0.3, (m, 3))
    boxes = as_boxes(c - h, c + h)
    a = near(15, 0.05)
    tris = np.zeros((m, 12), F)
    tris[:, 0:3] = a; tris[:, 4:7] = a + rng.uniform(-0.4, 0.4, (m, 3)); tris[:, 8:11] = a + rng.uniform(-0.4, 0.4, (m, 3))
    _CACHE[key] = dict(points=points, sweeps=sweeps, boxes=boxes, tris=tris)
    return _CACHE[key]
