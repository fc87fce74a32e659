"""Bad instance records (include/rt_api.h, rt_set_instances; DESIGN.md §5 "Instance records"): the case table, the scenes, the twin of
a scene and the query records of tests/test_instance_records.py.  No GPU is needed here.

A case is a function from a good record to a bad one.  Three classes:
  void            an entry of the transform is not finite, or the padded world box reaches 1e37: the record behaves like mask 0
  noninvertible   the transform is finite and its inverse is not: no ray hits it, the world-space queries keep its o2w image
  far             finite and below the limit (1e30): a valid record; the REST of the scene answers as without it
The twin of a scene is the same record array with every bad record's mask byte cleared and its transform set to the identity: what the
bad scene has to equal, output buffer for output buffer."""
import os

import numpy as np

from tests import scenes
from vulkan_raytracing_amd.api import INSTANCE_DTYPE

RES = scenes.RES
FLT_MAX = np.float32(3.4028234663852886e38)
N_RAYS, N_RECORDS = 4096, 512           # probe rays; points, sweeps, boxes and query triangles
FRAME_W, FRAME_H, SPP, BOUNCES = 96, 64, 2, 2
TRANSLATION = (3, 7, 11)
ROTATION = (0, 1, 2, 4, 5, 6, 8, 9, 10)
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


def _set(slot, value):
    def f(r):
        r = r.copy(); r["transform"][slot] = value; return r
    return f


def _matrix(rows, mask=None):
    def f(r):
        r = r.copy()
        t = np.asarray(r["transform"], np.float32).reshape(3, 4).copy()
        t[:, :3] = np.asarray(rows, np.float32)
        r["transform"] = t.reshape(12)
        if mask is not None:
            r["custom_index_and_mask"] = (int(r["custom_index_and_mask"]) & 0xFFFFFF) | (mask << 24)
        return r
    return f


def _all(value):
    def f(r):
        r = r.copy(); r["transform"] = value; return r
    return f


def _bytes_ff(r):
    """the 48 transform bytes 0xFF (a NaN in every slot), mask and mesh as they were"""
    r = r.copy()
    r["transform"] = np.frombuffer(b"\xff" * 48, np.float32)
    return r


def _scaled(s):
    def f(r):
        r = r.copy()
        t = np.asarray(r["transform"], np.float32).reshape(3, 4).copy()
        t[:, :3] *= np.float32(s)
        r["transform"] = t.reshape(12)
        return r
    return f


# name -> (function of the record, ...): more than one function makes that many CONSECUTIVE records bad, from the scene's bad index on
VOID = {"nan_slots": tuple(_set(k, np.nan) for k in range(12)),
        "rot_pinf": (_set(5, np.inf),), "rot_ninf": (_set(2, -np.inf),),
        "tr_pinf": (_set(3, np.inf),), "tr_ninf": (_set(11, -np.inf),),
        "all_nan": (_all(np.nan),), "bytes_ff": (_bytes_ff,),
        "tr_1e37": (_set(3, 1e37),), "tr_3e38": (_set(7, 3e38),), "tr_fltmax": (_set(11, FLT_MAX),)}
NONINVERTIBLE = {"rank2": (_matrix([[1, 0, 0], [0, 0, 0], [0, 0, 1]]),),
                 "rank1": (_matrix([[1, 2, 3], [2, 4, 6], [-1, -2, -3]]),),
                 "rank0": (_matrix(np.zeros((3, 3)), mask=0xFF),),
                 "scale_1e-40": (_scaled(1e-40),)}
FAR = {"tr_1e30": (_set(3, 1e30),), "tr_-1e30": (_set(7, -1e30),)}
CLASSES = {"void": VOID, "noninvertible": NONINVERTIBLE, "far": FAR}

# name -> (records, ring radius, bad record): the teapot (mirror) at the origin as record 0, cubes on a ring about it
SCENES = {"n1": (1, 5.0, 0), "n2_first": (2, 5.0, 0), "n2_second": (2, 5.0, 1), "n5": (5, 5.0, 2), "n300": (300, 120.0, 150)}

_CACHE = {}


def scene(name, ctx=None):
    """the ScenePair of SCENES[name] (cached without a context), all records good"""
    n, radius, _ = SCENES[name]
    make = lambda c: scenes.ring_scene(os.path.join(RES, "cube.obj"), n - 1, radius, BOUNCES, SPP, sky=scenes.synthetic_skybox(64), ctx=c,
                                       center_path=os.path.join(RES, "teapot.obj"))
    if ctx is not None:
        return make(ctx)
    if name not in _CACHE:
        _CACHE[name] = make(None)
    return _CACHE[name]


def bad_indices(name, fns):
    """the records the case makes bad: len(fns) consecutive ones from the scene's bad index on, as far as the scene has them"""
    n, _, b = SCENES[name]
    return list(range(b, min(n, b + len(fns))))


def bad_records(inst, name, fns):
    out = np.array(inst, INSTANCE_DTYPE).copy()
    for k, i in enumerate(bad_indices(name, fns)):
        out[i] = fns[k](out[i])
    return out


def twin_records(inst, bad):
    out = np.array(inst, INSTANCE_DTYPE).copy()
    for i in bad:
        out[i]["transform"] = IDENTITY
        out[i]["custom_index_and_mask"] = int(out[i]["custom_index_and_mask"]) & 0xFFFFFF
    return out


def centres(inst):
    return np.asarray(inst["transform"], np.float64)[:, TRANSLATION]


def probe_rays(name, seed=1):
    """N_RAYS aimed rays: ray i targets the centre of record i % n plus a uniform offset in [-0.5, 0.5]^3, from a sphere of radius
    3 * radius + 10 about the origin; tmin 0.001, tmax 10000"""
    n, radius, _ = SCENES[name]
    rng = np.random.default_rng(seed)
    tgt = centres(scene(name).instances)[np.arange(N_RAYS) % n] + rng.uniform(-0.5, 0.5, (N_RAYS, 3))
    o = rng.normal(size=(N_RAYS, 3)); o *= (3 * radius + 10) / np.linalg.norm(o, axis=1, keepdims=True)
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((N_RAYS, 8), np.float32)
    rays[:, 0:3] = o; rays[:, 3] = 0.001; rays[:, 4:7] = d; rays[:, 7] = 10000.0
    return rays


def targets(name, m, seed):
    """m points about the record centres, as probe_rays aims them (offsets up to 1.5: inside, on and outside the cubes)"""
    n = SCENES[name][0]
    rng = np.random.default_rng(seed)
    return centres(scene(name).instances)[np.arange(m) % n] + rng.uniform(-1.5, 1.5, (m, 3))


def query_records(name):
    """the other consumers' records, derived from the same targets with the generators' own record layouts (tests/test_closest_point.py
    with_radius, test_sphere_sweep.py as_sweeps, test_overlap_boxes.py as_boxes, api.triangle_records' 12 floats)"""
    from tests.test_closest_point import with_radius
    from tests.test_overlap_boxes import as_boxes
    from tests.test_sphere_sweep import as_sweeps, unit
    key = ("records", name)
    if key in _CACHE:
        return _CACHE[key]
    n, radius, _ = SCENES[name]
    m = N_RECORDS
    rng = np.random.default_rng(11)
    p = targets(name, m, 12)
    points = with_radius(p, np.where(np.arange(m) % 4 == 0, 1.0, np.inf))
    o = unit(rng.normal(size=(m, 3))) * (3 * radius + 10)
    tgt = targets(name, m, 13)
    sweeps = as_sweeps(o, 10 ** rng.uniform(-2, -0.3, m), unit(tgt - o), np.where(np.arange(m) % 3 == 0, np.inf, 4 * radius + 10))
    c = targets(name, m, 14)
    h = 10 ** rng.uniform(-2, 0, (m, 3))
    boxes = as_boxes(c - h, c + h)
    a = targets(name, m, 15)
    tris = np.zeros((m, 12), np.float32)
    tris[:, 0:3] = a; tris[:, 4:7] = a + rng.uniform(-1, 1, (m, 3)); tris[:, 8:11] = a + rng.uniform(-1, 1, (m, 3))
    _CACHE[key] = dict(points=points, sweeps=sweeps, boxes=boxes, tris=tris)
    return _CACHE[key]
