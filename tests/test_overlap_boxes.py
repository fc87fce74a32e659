"""rt_overlap_boxes_device / rt_overlap_boxes: the triangles of the scene that touch every query box.

tests/overlap_reference.py holds the two references: brute32, the canonical binary32 predicate of include/rt_api.h and DESIGN.md §5 "Box
overlaps" restated in numpy over every (box, instance, triangle) pair, and brute64, the same thirteen axes in binary64 on the same
binary32 inputs.  The CPU part holds brute32 to brute64 (they may differ only on pairs within REL of the decision boundary, on at most 1 %
of the intersecting-or-near pairs of a set, and not at all on the integer lattice); the GPU part holds the library to brute32 bit for bit:
counts and id rows, under every tree the library can build, far from the origin, on degenerate geometry, with touching voxels, every
max_ids mode, and the plumbing of a device query."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import closest_reference as cr
from tests import overlap_reference as orf
from tests import scenes
from tests.query_reference import REL
from tests.test_closest_point import degenerate_soup, scene_box, small_scene, surface_points, teapot_scene
from tests.test_ray_query import PATHS, dev_inst, slow_queue
from tests.test_ray_query_oracle import placed_instances, small_meshes, use_builder
from vulkan_raytracing_amd import RtContext, api
from vulkan_raytracing_amd.api import RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2


# ---- scenes and box sets ------------------------------------------------------------------------------------------------------

def as_boxes(lo, hi):
    b = np.zeros((len(lo), 8), np.float32)
    b[:, 0:3] = lo; b[:, 4:7] = hi
    b[:, 3] = 7.0; b[:, 7] = np.nan   # (words 3 and 7 are ignored)
    return b


def invalid_boxes(b):
    """records the contract answers with count 0: NaN / inf bounds, lo > hi on an axis"""
    q = np.array(b[:10], np.float32).copy()
    q[0, 0] = np.nan; q[1, 5] = np.inf; q[2, 2] = -np.inf; q[3, 4] = np.nan
    q[4, [0, 4]] = q[4, [4, 0]] + np.float32([1, 0]); q[5, [1, 5]] = [2.0, 1.0]; q[6, [2, 6]] = [0.5, -0.5]
    q[7, 0:3] = -np.inf; q[7, 4:7] = np.inf
    return q


def aspect(sc):
    """(triangles,) the height over the longest edge divided by that edge (0 for zero-area triangles), binary64"""
    e = [sc.B - sc.A, sc.C - sc.B, sc.A - sc.C]
    longest = np.max([np.linalg.norm(x, axis=1) for x in e], axis=0)
    area2 = np.linalg.norm(np.cross(e[0], -e[2]), axis=1)
    return area2 / np.where(longest > 0, longest * longest, 1.0)


def box_sets(sc, tris, seed, n=2000, resolvable=0.0):
    """three sets of 2 000 to 2 200 boxes: `mixed` (random boxes from a thousandth of the scene size to the whole scene, one box that
    encloses everything, boxes far outside, invalid records), `surface` (tiny boxes centred on surface points), `features` (lo == hi on
    all axes at vertices and on edges, and on one or two axes: planes and lines through surface points).
    What binary32 can resolve bounds the tiny boxes from below: no extent that is not collapsed is under 2^-14 of the largest coordinate
    (1 024 ulps: 10 000 units out a smaller box is not the box that was asked for) nor under `resolvable` (the soup: ten times its
    needles' width).  Boxes with a collapsed axis decide on exact ties, so they sit on triangles of aspect above 0.01 only (a needle's
    edge axes are rounding noise at zero extent); such a box may still touch a needle that crosses it."""
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(sc)
    c, ext = (lo + hi) / 2, hi - lo
    floor = max(2.0 ** -14 * max(np.abs(lo).max(), np.abs(hi).max()), resolvable)
    fat = np.nonzero(aspect(sc) > 0.01)[0]
    size = ext.max() * 10 ** rng.uniform(-3, 0, (n, 1)) * rng.uniform(0.3, 1.0, (n, 3))
    ctr = c + rng.uniform(-0.55, 0.55, (n, 3)) * ext
    far = c + rng.choice([-1.0, 1.0], (100, 3)) * ext * rng.uniform(3, 50, (100, 3))
    mixed = np.concatenate([as_boxes(ctr - size / 2, ctr + size / 2), as_boxes(lo[None] - 1, hi[None] + 1), as_boxes(far - 0.1 * ext, far + 0.1 * ext)])
    mixed = np.concatenate([mixed, invalid_boxes(mixed)])
    mixed = mixed[rng.permutation(len(mixed))]
    # (centred on triangles with an area: the plane axis of a collinear triangle is a rounding residue in binary32 and exactly nothing in
    # binary64; the zero-area triangles are still there to be crossed, and test_restatement_edge_cases has them)
    area = np.nonzero(aspect(sc) > 1e-6)[0]
    ka = area[rng.integers(0, len(area), n)]
    uv = rng.dirichlet([1, 1, 1], n)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = uv[:, 0:1] * sc.A[ka] + uv[:, 1:2] * sc.B[ka] + uv[:, 2:3] * sc.C[ka] + d * rng.uniform(0, 1e-3 * ext.max(), (n, 1))
    s = np.maximum(ext.max() * 10 ** rng.uniform(-4, -2, (n, 1)) * rng.uniform(0.3, 1.0, (n, 3)), floor)
    surface = as_boxes(p - s, p + s)
    k = fat[rng.integers(0, len(fat), n)]
    # (the binary32 vertices the predicate forms; mostly A: the plane axis takes d = dot3(n, A - c), which is exactly 0 only there, and a
    # point box has r = 0 on every axis, so at B and C the binary32 answer hangs on the rounding of d: DESIGN.md §5)
    on_v = np.where((k % 8 != 0)[:, None], tris.A[k], np.where((k % 16 == 0)[:, None], tris.B[k], tris.C[k]))
    t = rng.uniform(size=(n, 1))
    on_e = sc.A[k] + t * (sc.B[k] - sc.A[k])
    kf = fat[rng.integers(0, len(fat), n)]
    uv = rng.dirichlet([1, 1, 1], n)
    flat = uv[:, 0:1] * sc.A[kf] + uv[:, 1:2] * sc.B[kf] + uv[:, 2:3] * sc.C[kf]
    fl, fh = flat - s * 20, flat + s * 20
    axes = rng.integers(1, 7, n)   # which axes collapse: one or two of them
    for a in range(3):
        m = (axes >> a) & 1 == 1
        fl[m, a] = flat[m, a]; fh[m, a] = flat[m, a]
    q = n // 20   # (point boxes decide on exact ties: few of them, so that the 1 % cap on binary32 / binary64 disagreements holds per set)
    features = np.concatenate([as_boxes(on_v[:q], on_v[:q]), as_boxes(on_e[:q], on_e[:q]), as_boxes(fl[:n - 2 * q], fh[:n - 2 * q])])
    return {"mixed": mixed, "surface": surface, "features": features}


def lattice_scene():
    """a height field and an octahedron with every vertex on the integer lattice, under identity and pure integer translations: every
    operation of the predicate is exact there, in binary32 and binary64 alike"""
    rng = np.random.default_rng(171)
    g = 7
    z = rng.integers(-2, 3, (g, g))
    P = [[i, j, z[i, j]] for i in range(g) for j in range(g)]
    tris = []
    for i in range(g - 1):
        for j in range(g - 1):
            a, b, c, d = i * g + j, (i + 1) * g + j, (i + 1) * g + j + 1, i * g + j + 1
            tris += [[a, b, c], [a, c, d]] if (i + j) % 2 else [[a, b, d], [b, c, d]]
    n0 = len(P)
    P += [[2, 0, 0], [-2, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 2], [0, 0, -2]]
    octa = [[n0 + a, n0 + b, n0 + c] for a in (0, 1) for b in (2, 3) for c in (4, 5)]
    pos = np.array(P, np.float32)
    verts = np.concatenate([pos, np.tile([[0, 0, 1]], (len(pos), 1))], axis=1).astype(np.float32).reshape(-1)
    idx = np.array(tris + octa, np.uint32).reshape(-1)
    ranges = [(0, 0, len(tris)), (0, 3 * len(tris), len(octa))]
    inst = np.zeros(5, api.INSTANCE_DTYPE)
    for i, (mesh, t) in enumerate([(0, (0, 0, 0)), (1, (3, 3, 0)), (0, (-8, 2, 1)), (1, (-5, -4, 3)), (1, (3, 3, 1))]):
        inst[i]["transform"] = np.array([1, 0, 0, t[0], 0, 1, 0, t[1], 0, 0, 1, t[2]], np.float32)
        inst[i]["custom_index_and_mask"] = i | (0xFF << 24)
        inst[i]["mesh"] = mesh
    return verts, idx, ranges, inst


def lattice_voxels():
    """unit voxels whose faces pass through the lattice: 16 x 14 x 9 = 2016 of them around lattice_scene"""
    x, y, z = np.meshgrid(np.arange(-9, 7), np.arange(-7, 7), np.arange(-4, 5), indexing="ij")
    lo = np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(np.float32)
    return as_boxes(lo, lo + 1)


def cancelling_scene(seed=181, offset=4096.0):
    """small_meshes moved `offset` away from the object-space origin under instances whose translations bring them back: the world
    coordinates are small, the terms of a = xform_point(o2w, v0) large"""
    verts, idx, ranges = small_meshes(seed)
    v = verts.reshape(-1, 6).copy()
    v[:, :3] += np.float32(offset)
    inst = placed_instances(16, seed + 1, spacing=3.0)
    for i in range(len(inst)):
        M = np.asarray(inst[i]["transform"], np.float64).reshape(3, 4)
        M[:, 3] -= M[:, :3] @ np.full(3, offset)
        inst[i]["transform"] = M.astype(np.float32).reshape(12)
    return v.reshape(-1), idx, ranges, inst


def sliver_scene(seed=191):
    """long slivers (aspect 1e-4) that are axis-aligned in object space, under rotated, sheared and mirrored instances: the object-space
    boxes of the walk hug them, and the binary32 edge and plane axes of a sliver are at their least exact"""
    rng = np.random.default_rng(seed)
    pos = []
    for k in range(12):
        a = rng.uniform(-1, 1, 3)
        ax, up = k % 3, (k + 1 + k // 3 % 2) % 3
        b, c = a.copy(), a.copy()
        b[ax] += 4.0
        c[ax] += rng.uniform(1.0, 3.0); c[up] += 4e-4
        pos += [a, b, c]
    for k in range(2):   # (and two ordinary triangles)
        a = rng.uniform(-1, 1, 3)
        pos += [a, a + rng.uniform(-1, 1, 3), a + rng.uniform(-1, 1, 3)]
    pos = np.array(pos, np.float32)
    verts = np.concatenate([pos, np.tile([[0, 0, 1]], (len(pos), 1))], axis=1).astype(np.float32).reshape(-1)
    return verts, np.arange(len(pos), dtype=np.uint32), [(0, 0, 14)], placed_instances(12, seed + 1, spacing=4.0, n_meshes=1)


SCENES = {"sliver": sliver_scene, "small": lambda: small_scene(seed=151), "teapot": teapot_scene,
          "soup": lambda: degenerate_soup(62) + (placed_instances(12, 63, spacing=2.5, n_meshes=1),)}
_CACHE = {}


def scene_and_sets(name):
    """the scene, its Triangles, its box sets and brute32 of every set at max_ids 16, computed once"""
    if name not in _CACHE:
        if name == "lattice":
            parts = lattice_scene()
        elif name == "cancel":
            parts = cancelling_scene()
        elif name.startswith("small+"):
            parts = small_scene(seed=161, offset=float(name[6:]))
        else:
            parts = SCENES[name]()
        sc = cr.Scene(*parts)
        tris = orf.Triangles(sc)
        # (the soup's needles are 1e-4 wide, the slivers 4e-4: a hundred times that)
        sets = {"voxels": lattice_voxels()} if name == "lattice" else box_sets(sc, tris, seed=152, resolvable={"soup": 1e-2, "sliver": 4e-2}.get(name, 0.0))
        ref = {k: orf.brute32(sc, b, tris=tris) for k, b in sets.items()}
        _CACHE[name] = (parts, sc, tris, sets, ref)
    return _CACHE[name]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_exports_abi_and_null_context():
    assert "rt_overlap_boxes_device" in api.EXPORTS and "rt_overlap_boxes" in api.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^#define RT_OVERLAP_ANY 0x1u$", hdr, re.M)
    assert re.search(r"^int rt_overlap_boxes_device\(rt_ctx\* ctx, size_t n, const void\* d_boxes8, uint32_t cull_mask, uint32_t flags,\s+uint32_t max_ids, "
                     r"void\* d_ids, void\* d_counts, void\* hip_stream\);", hdr, re.M)
    assert re.search(r"^int rt_overlap_boxes\(rt_ctx\* ctx, size_t n, const float\* boxes8_host, uint32_t cull_mask, uint32_t flags,\s+uint32_t max_ids, "
                     r"int32_t\* ids_host, uint32_t\* counts_host, int counting, rt_stats\* stats\);", hdr, re.M)
    L = api.lib()
    assert hasattr(L, "rt_overlap_boxes_device") and hasattr(L, "rt_overlap_boxes") and L.rt_abi_version() == 7
    assert L.rt_overlap_boxes_device(None, 0, None, 0xFF, 0, 0, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_overlap_boxes_device(None, 64, None, 0xFF, 0, 4, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_overlap_boxes(None, 0, None, 0xFF, 0, 0, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert hasattr(RtContext, "overlap_boxes_device") and hasattr(RtContext, "overlap_boxes")


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_overlap_kernels_keep_the_record_level_budget(target):
    """exactly two new walk kernels, k_overlap_boxes and its counting form, in both libraries, each within the record-level walks' budget
    (>= 4 waves per SIMD, scratch <= 32 bytes, no spills)"""
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    walk = [(n, r) for n, r in kernels.items() if "k_overlap" in n]
    assert len(walk) == 2 and sum("k_overlap_boxes_count" in n for n, _ in walk) == 1 and all("k_overlap_boxes" in n for n, _ in walk), "\n".join(kernels)
    for name, r in walk:
        assert int(r["Occupancy"]) >= 4 and int(r["ScratchSize"]) <= 32 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)


@pytest.mark.parametrize("name", ["small", "teapot", "soup", "sliver", "small+1000", "small+10000", "cancel", "lattice"])
def test_binary32_restatement_against_binary64(name):
    """every pair on which brute32 and brute64 disagree has a binary64 separation within REL of zero, and such pairs are at most 1 % of
    the set's intersecting-or-near pairs (binary64 candidates and pairs separated by at most REL); on the integer lattice none disagree.
    Every set of every scene of the GPU tests."""
    parts, sc, tris, sets, ref = scene_and_sets(name)
    for k, boxes in sets.items():
        bi, ti = orf.surviving_pairs(tris, boxes)
        c32 = orf.candidates32(tris, boxes, bi, ti)
        s64 = orf.separation64(tris, boxes, bi, ti)
        differ = c32 != (s64 <= 0)
        near = np.abs(s64) <= REL
        pool = (s64 <= 0) | near
        print("%s %s: %d pairs past the box axes, %d intersecting or near, %d near, %d differ (worst |separation| %.3g)" %
              (name, k, len(bi), pool.sum(), near.sum(), differ.sum(), np.abs(s64[differ]).max() if differ.any() else 0.0))
        assert (ref[k][0] == np.bincount(bi[c32], minlength=len(boxes))).all()
        if name == "lattice":
            assert not differ.any()
            continue
        assert near[differ].all(), (k, np.abs(s64[differ]).max())
        assert differ.sum() <= 0.01 * pool.sum(), (k, differ.sum(), pool.sum())


def test_restatement_edge_cases():
    """invalid records, lo == hi boxes, cull masks that exclude every instance, a zero-area triangle"""
    parts, sc, tris, sets, ref = scene_and_sets("small")
    mixed = sets["mixed"]
    bad = invalid_boxes(sets["surface"])
    assert not orf.valid_boxes(bad)[:8].any() and orf.valid_boxes(bad)[8:].all()
    counts, ids = orf.brute32(sc, bad, tris=tris)
    assert (counts[:8] == 0).all() and (ids[:8] == -1).all()
    # the enclosing box lists every triangle of every instance the mask admits
    big = as_boxes(scene_box(sc)[0][None] - 1, scene_box(sc)[1][None] + 1)
    for cull in (0xFF, 0x01, 0x5A):
        counts, ids = orf.brute32(sc, big, cull, tris=tris)
        adm = sc.admitted(cull)
        assert counts[0] == adm.sum() and (ids[0, :, 0] == sc.inst[adm][:16]).all() and (ids[0, :, 1] == sc.prim[adm][:16]).all()
    assert (orf.brute32(sc, mixed, 0, tris=tris)[0] == 0).all()
    # a point box on a vertex touches every triangle that holds that vertex as its A; one a little off it touches none of them
    k = np.nonzero(sc.admitted(0xFF))[0][::7]
    at = as_boxes(tris.A[k], tris.A[k])
    counts, ids = orf.brute32(sc, at, tris=tris)
    own = np.stack([sc.inst[k], sc.prim[k]], axis=1)
    assert (counts >= 1).all() and all((ids[i] == own[i]).all(axis=1).any() for i in range(len(k)))
    # zero-area triangles (two equal vertices, collinear ones, a point): a point box on the vertex finds them, the plane separates nothing
    parts, sc, tris, sets, ref = scene_and_sets("soup")
    deg = np.nonzero((sc.prim % 6 == 3) & sc.admitted(0xFF))[0]   # (a, a, a)
    counts, ids = orf.brute32(sc, as_boxes(tris.A[deg], tris.A[deg]), tris=tris)
    own = np.stack([sc.inst[deg], sc.prim[deg]], axis=1)
    assert all((ids[i] == own[i]).all(axis=1).any() for i in range(len(deg)))
    far = orf.brute32(sc, as_boxes(tris.A[deg] + 50, tris.A[deg] + 51), tris=tris)[0]
    assert (far == 0).all()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


def dev(b):
    import torch
    return torch.from_numpy(np.ascontiguousarray(b, np.float32).reshape(-1, 8)).to("cuda:0")


def gpu_overlap(c, boxes, max_ids=16, cull=0xFF, counts=True, any=False):
    import torch
    res = c.overlap_boxes_device(dev(boxes), max_ids=max_ids, cull_mask=cull, counts=counts, any=any)
    torch.cuda.synchronize()
    return res.numpy()


def check(got, ref, what, max_ids=16):
    """(counts, ids) of the GPU against brute32's at max_ids 16, bit for bit"""
    counts, ids = got
    rc, ri = ref
    if counts is not None and counts.tobytes() != rc.tobytes():
        bad = np.nonzero(counts != rc)[0]
        raise AssertionError("%s: %d counts differ from the brute force, first box %d: gpu %d reference %d" % (what, len(bad), bad[0], counts[bad[0]], rc[bad[0]]))
    if max_ids:
        want = np.ascontiguousarray(ri[:, :max_ids])
        if ids.tobytes() != want.tobytes():
            bad = np.nonzero((ids != want).any(axis=(1, 2)))[0]
            raise AssertionError("%s: %d rows differ from the brute force, first box %d: gpu %s reference %s" % (what, len(bad), bad[0], ids[bad[0]].tolist(), want[bad[0]].tolist()))
    else:
        assert ids is None, what


def load(c, parts):
    verts, idx, ranges, inst = parts
    c.upload_geometry(verts, idx, ranges)
    c.set_instances(inst)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "teapot", "soup", "sliver"])
def test_every_box_set(ctx, name):
    """random boxes of every size, tiny boxes on the surface, lo == hi boxes, the enclosing box (through the spill stack), boxes far
    outside, invalid records; cull masks"""
    parts, sc, tris, sets, ref = scene_and_sets(name)
    load(ctx, parts)
    for k, boxes in sets.items():
        check(gpu_overlap(ctx, boxes), ref[k], "%s %s" % (name, k))
    mixed = sets["mixed"]
    big = np.nonzero(ref["mixed"][0] == ref["mixed"][0].max())[0][0]
    assert ref["mixed"][0][big] == sc.admitted(0xFF).sum() > 0   # the enclosing box: every triangle of every unmasked instance
    assert (ref["mixed"][0][~orf.valid_boxes(mixed)] == 0).all() and (~orf.valid_boxes(mixed)).sum() >= 8
    for cull in (0x01, 0x5A, 0x00):
        r = orf.brute32(sc, mixed, cull, tris=tris)
        check(gpu_overlap(ctx, mixed, cull=cull), r, "%s mixed cull %#x" % (name, cull))
        assert r[0][big] == sc.admitted(cull).sum()


@pytest.mark.gpu
def test_touching_voxels_on_the_integer_lattice(ctx):
    """unit voxels whose faces pass through the vertices of a lattice mesh: closed sets, exact answers"""
    parts, sc, tris, sets, ref = scene_and_sets("lattice")
    load(ctx, parts)
    boxes = sets["voxels"]
    check(gpu_overlap(ctx, boxes), ref["voxels"], "lattice voxels")
    r64 = orf.brute64(sc, boxes, tris=tris)
    assert r64[0].tobytes() == ref["voxels"][0].tobytes() and r64[1].tobytes() == ref["voxels"][1].tobytes()
    # a voxel that only touches: a vertex of the height field at a corner of the voxel
    assert (ref["voxels"][0] > 0).sum() > 300
    occ = gpu_overlap(ctx, boxes, max_ids=0, any=True)[0]
    assert np.array_equal(occ, (ref["voxels"][0] > 0).astype(np.uint32))


@pytest.mark.gpu
def test_max_ids_counts_pruning_and_any(ctx):
    """max_ids 0, 1, 3, 16 on boxes with more candidates than that, with and without counts (the pruning path): the same rows;
    RT_OVERLAP_ANY equals count > 0"""
    parts, sc, tris, sets, ref = scene_and_sets("small")
    load(ctx, parts)
    rc, ri = ref["mixed"]
    many = np.nonzero(rc > 16)[0]
    assert len(many) >= 100
    boxes = np.concatenate([sets["mixed"][many], sets["mixed"][:500]])
    r = (np.concatenate([rc[many], rc[:500]]), np.concatenate([ri[many], ri[:500]]))
    for k in (0, 1, 3, 16):
        check(gpu_overlap(ctx, boxes, max_ids=k), r, "max_ids %d with counts" % k, max_ids=k)
        if k:
            counts, ids = gpu_overlap(ctx, boxes, max_ids=k, counts=False)
            assert counts is None
            check((None, ids), r, "max_ids %d without counts" % k, max_ids=k)
    for name, b in sets.items():
        occ, ids = gpu_overlap(ctx, b, max_ids=0, any=True)
        assert ids is None and np.array_equal(occ, (ref[name][0] > 0).astype(np.uint32)), name
    occ = gpu_overlap(ctx, boxes, max_ids=0, any=True, cull=0x02)[0]
    assert np.array_equal(occ, (orf.brute32(sc, boxes, 0x02, tris=tris)[0] > 0).astype(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "unset", "1", "2"])
def test_tree_independence(builder, monkeypatch):
    """the same boxes over blas_builder 0 and RT_GPU_BVH_ALGO unset / 1 / 2, host and device instance records with their refits: every
    output equals one brute force, so they are byte-identical to each other"""
    import torch
    parts, sc0, tris0, sets, ref = scene_and_sets("small")
    verts, idx, ranges, inst = parts
    rng = np.random.default_rng(72)
    moved = inst.copy()
    moved["transform"][:, [3, 7, 11]] += rng.uniform(-0.3, 0.3, (len(inst), 3)).astype(np.float32)
    boxes = np.concatenate([sets["mixed"][:1200], sets["surface"][:600], sets["features"][:600]])
    r0 = tuple(np.concatenate([ref["mixed"][j][:1200], ref["surface"][j][:600], ref["features"][j][:600]]) for j in (0, 1))
    sc1 = cr.Scene(verts, idx, ranges, moved)
    r1 = orf.brute32(sc1, boxes)
    c = RtContext(0)
    try:
        if builder == "unset":
            monkeypatch.delenv("RT_GPU_BVH_ALGO", raising=False)
            c.set_param("blas_builder", 1)
        else:
            use_builder(c, builder, monkeypatch)
        c.upload_geometry(verts, idx, ranges)
        for source in ("host", "device"):
            for records, update, r in ((inst, False, r0), (moved, True, r1)):
                if source == "host":
                    c.set_instances(records, update=update)
                else:
                    torch.cuda.synchronize()
                    c.set_instances_device(dev_inst(records), update=update)
                what = "%s records, update %d, builder %s" % (source, update, builder)
                check(gpu_overlap(c, boxes), r, what)
                check(gpu_overlap(c, boxes, max_ids=3, counts=False), r, what + ", pruning", max_ids=3)
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small+1000", "small+10000", "cancel"])
def test_translated_and_cancelling_scenes(ctx, name):
    """the scene 1 000 and 10 000 units from the origin, and instances whose translation cancels their mesh's own offset: the walk's
    slack must cover the rounding of the world vertices"""
    parts, sc, tris, sets, ref = scene_and_sets(name)
    load(ctx, parts)
    for k, boxes in sets.items():
        check(gpu_overlap(ctx, boxes), ref[k], "%s %s" % (name, k))
    assert (ref["surface"][0] > 0).mean() > 0.5


@pytest.mark.gpu
def test_refit_then_tlas_update_equals_a_fresh_build():
    import torch
    from tests.test_blas_refit import deform, with_mesh
    parts, sc0, tris0, sets, ref = scene_and_sets("small")
    verts, idx, ranges, inst = parts
    geom = types.SimpleNamespace(verts=verts, idx=idx, ranges=ranges)
    boxes = np.concatenate([sets["mixed"][:1500], sets["surface"][:800]])
    src = dev(boxes)
    c, fresh = RtContext(0), RtContext(0)
    try:
        load(c, parts)
        t = deform(geom, 0, amp=0.2)
        torch.cuda.synchronize()
        c.refit_blas_device(0, t)
        torch.cuda.synchronize()
        ids = torch.empty((len(boxes), 16, 2), dtype=torch.int32, device="cuda:0")
        rc = c.L.rt_overlap_boxes_device(c.h, len(boxes), ctypes.c_void_p(src.data_ptr()), 0xFF, 0, 16, ctypes.c_void_p(ids.data_ptr()), None, None)
        assert rc == RT_ERR_NOT_READY
        c.set_instances_device(dev_inst(inst))
        v2 = with_mesh(geom, verts, 0, t)
        load(fresh, (v2, idx, ranges, inst))
        got, want = gpu_overlap(c, boxes), gpu_overlap(fresh, boxes)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        check(got, orf.brute32(cr.Scene(v2, idx, ranges, inst), boxes), "after the refit")
    finally:
        c.close()
        fresh.close()


@pytest.mark.gpu
def test_plumbing(ctx):
    """a caller's stream with the boxes written by a kernel queued just before the call; out= reuse; host form = device form; counting
    fills the visit counters; n == 0"""
    import torch
    parts, sc, tris, sets, ref = scene_and_sets("small")
    load(ctx, parts)
    boxes = sets["mixed"]
    r = ref["mixed"]
    # host form
    cnt, ids, st = ctx.overlap_boxes(boxes, max_ids=16)
    check((cnt, ids), r, "host form")
    assert st.node_visits == 0 and st.tri_tests == 0
    cnt, ids, st = ctx.overlap_boxes(boxes, max_ids=16, counting=True)
    check((cnt, ids), r, "host form, counting")
    assert st.node_visits > 0 and st.tri_tests >= int(r[0].sum())
    cnt, ids, st = ctx.overlap_boxes(boxes, max_ids=0, counting=True)
    assert ids is None and cnt.tobytes() == r[0].tobytes()
    cnt, ids, st_any = ctx.overlap_boxes(boxes, max_ids=0, any=True, counting=True)
    assert np.array_equal(cnt, (r[0] > 0).astype(np.uint32)) and 0 < st_any.tri_tests <= st.tri_tests
    cnt, ids, _ = ctx.overlap_boxes(boxes, max_ids=3, counts=False)
    assert cnt is None
    check((None, ids), r, "host form without counts", max_ids=3)
    # out= reuse
    src = dev(boxes)
    ids_t = torch.empty((len(boxes), 16, 2), dtype=torch.int32, device="cuda:0"); cnt_t = torch.empty((len(boxes),), dtype=torch.int32, device="cuda:0")
    res = ctx.overlap_boxes_device(src, max_ids=16, out=(ids_t, cnt_t))
    assert res.ids.data_ptr() == ids_t.data_ptr() and res.count.data_ptr() == cnt_t.data_ptr()
    check(res.numpy(), r, "out= reuse")
    assert res.inst.shape == (len(boxes), 16) and res.prim.shape == (len(boxes), 16)
    with pytest.raises(ValueError):
        ctx.overlap_boxes_device(src, max_ids=16, out=(ids_t[:-1], cnt_t))
    # stream order: the boxes are made by a kernel behind a slow queue on a side stream, and overwritten right after the call
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = slow_queue(torch, 12)
        p = (src + (a[0, 0] != a[0, 0]).to(torch.float32) * 0).contiguous()   # made behind the queue, on s (NaN + 0 keeps word 7)
        r1 = ctx.overlap_boxes_device(p, max_ids=16, stream=s)
        r2 = ctx.overlap_boxes_device(p, max_ids=0, any=True, stream=s)
        p.zero_()
        i1, c1, c2 = r1.ids.clone(), r1.count.clone(), r2.count.clone()
    s.synchronize()
    check((c1.cpu().numpy().view(np.uint32), i1.cpu().numpy()), r, "stream order")
    assert np.array_equal(c2.cpu().numpy().view(np.uint32), (r[0] > 0).astype(np.uint32))
    # n == 0
    e = ctx.overlap_boxes_device(torch.empty((0, 8), dtype=torch.float32, device="cuda:0"), max_ids=4)
    assert e.ids.shape == (0, 4, 2) and e.count.shape == (0,)
    cnt, ids, _ = ctx.overlap_boxes(np.zeros((0, 8), np.float32), max_ids=2)
    assert len(cnt) == 0 and ids.shape == (0, 2, 2)


@pytest.mark.gpu
def test_frame_in_flight_beside_an_overlap_query():
    """a frame in flight on the context's slot is neither waited for nor changed: its pixels equal the frame rendered alone"""
    import torch
    from tests.test_ray_query import W, H, two_objects
    base = RtContext(0)
    slot = base.frame_slot()
    try:
        sp = two_objects(base)
        slot.set_instances(sp.instances)
        slot.set_uniforms(sp.uniforms)
        before = base.trace(W, H)[0]
        sc = cr.Scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances)
        rng = np.random.default_rng(111)
        p = surface_points(sc, 2000, rng, 0.0)
        lo, hi = scene_box(sc)
        h = (hi - lo).max() * 10 ** rng.uniform(-3, -1.5, (2000, 1))
        boxes = as_boxes(p - h, p + h)
        src = dev(boxes)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        slot.trace_async(W, H)
        with torch.cuda.stream(s):
            slow_queue(torch, 4)
            res = base.overlap_boxes_device(src, max_ids=16, stream=s)
        during, _ = slot.trace_wait()
        after = base.trace(W, H)[0]
        s.synchronize()
        assert np.array_equal(during.view(np.uint32), before.view(np.uint32))
        assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
        check(res.numpy(), orf.brute32(sc, boxes), "beside frames")
    finally:
        slot.close()
        base.close()


def _raw(c, n, boxes, cull, flags, k, ids, counts):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_overlap_boxes_device(c.h, n, p(boxes), cull, flags, k, p(ids), p(counts), None)


@pytest.mark.gpu
def test_error_statuses():
    import torch
    from tests.test_blas_refit import span
    sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
    sc = cr.Scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances)
    rng = np.random.default_rng(121)
    pts = surface_points(sc, 500, rng, 0.0)
    boxes_np = as_boxes(pts - 0.01, pts + 0.01)
    ref = orf.brute32(sc, boxes_np, max_ids=4)
    boxes = dev(boxes_np)
    n = boxes.shape[0]
    ids = torch.empty((n + 1, 4, 2), dtype=torch.int32, device="cuda:0")
    cnt = torch.empty((n + 1,), dtype=torch.int32, device="cuda:0")
    B_, I_, C_ = boxes.data_ptr(), ids.data_ptr(), cnt.data_ptr()
    c = RtContext(0)

    def err(args, code, text):
        assert _raw(c, *args) == code, args
        msg = c.L.rt_last_error(c.h).decode()
        assert text in msg, (args, msg)

    def ok():
        got = c.overlap_boxes_device(boxes, max_ids=4).numpy()
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()

    try:
        err((n, B_, 0xFF, 0, 4, I_, C_), RT_ERR_NOT_READY, "")   # no geometry
        c.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        err((n, B_, 0xFF, 0, 4, I_, C_), RT_ERR_NOT_READY, "")   # no TLAS
        c.set_instances(sp.instances)
        c.set_uniforms(sp.uniforms)
        ok()
        bad = [((0xFFFFFF00, B_, 0xFF, 0, 4, I_, C_), "too many boxes"), ((0x10000000, B_, 0xFF, 0, 16, I_, C_), "n * max_ids"),
               ((n, B_, 0x100, 0, 4, I_, C_), "cull_mask"), ((n, B_, 0xFF, 0x2, 4, I_, C_), "unknown flag bits"), ((n, B_, 0xFF, 0x80000000, 0, 0, C_), "unknown flag bits"),
               ((n, B_, 0xFF, 0, 17, I_, C_), "max_ids must be 0..16"), ((n, B_, 0xFF, 0, 0, I_, C_), "max_ids 0 counts only"), ((n, B_, 0xFF, 0, 0, I_, 0), "max_ids 0 counts only"),
               ((n, B_, 0xFF, 1, 4, I_, C_), "RT_OVERLAP_ANY needs max_ids 0"), ((n, B_, 0xFF, 1, 0, 0, 0), "neither ids nor counts"),
               ((n, B_, 0xFF, 0, 4, 0, 0), "neither ids nor counts"), ((n, B_, 0xFF, 0, 4, 0, C_), "null id pointer"), ((n, 0, 0xFF, 0, 4, I_, C_), "null box pointer"),
               ((n, B_ + 4, 0xFF, 0, 4, I_, C_), "aligned"), ((n, B_, 0xFF, 0, 4, I_ + 2, C_), "aligned"), ((n, B_, 0xFF, 0, 4, I_, C_ + 1), "aligned")]
        host_buf = np.zeros((n + 1, 8), np.float32)
        pinned = torch.zeros((n, 8), dtype=torch.float32).pin_memory()
        for ptr in ((host_buf.ctypes.data + 15) & ~15, pinned.data_ptr()):   # (16-byte aligned: only the memory kind is wrong)
            bad += [((n, ptr, 0xFF, 0, 4, I_, C_), "device memory of the context's GPU"), ((n, B_, 0xFF, 0, 4, ptr, C_), "device memory of the context's GPU"),
                    ((n, B_, 0xFF, 0, 4, I_, ptr), "device memory of the context's GPU")]
        for args, text in bad:
            err(args, RT_ERR_INVALID_ARGUMENT, text)
            ok()
        # 4-byte aligned rows and counts that are not 8- or 16-byte aligned are fine
        assert _raw(c, n, B_, 0xFF, 0, 4, I_ + 4, C_ + 4) == 0
        torch.cuda.synchronize()
        assert ids.view(-1)[1:1 + 8 * n].cpu().numpy().tobytes() == ref[1].tobytes() and cnt[1:].cpu().numpy().view(np.uint32).tobytes() == ref[0].tobytes()
        out_c = np.zeros(n, np.uint32)
        P = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        assert c.L.rt_overlap_boxes(c.h, n, None, 0xFF, 0, 0, None, P(out_c), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_overlap_boxes(c.h, n, P(boxes_np), 0x100, 0, 0, None, P(out_c), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_overlap_boxes(c.h, n, P(boxes_np), 0xFF, 1, 2, None, P(out_c), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_overlap_boxes(c.h, n, P(boxes_np), 0xFF, 0, 0, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
        ok()
        assert _raw(c, 0, 0, 0xFF, 0, 0, 0, C_) == 0   # n == 0 enqueues nothing and needs no box pointer
        with pytest.raises(ValueError):
            c.overlap_boxes_device(boxes.cpu())
        with pytest.raises(ValueError):
            c.overlap_boxes_device(torch.zeros((4, 4), dtype=torch.float32, device="cuda:0"))
        with pytest.raises(ValueError):
            c.overlap_boxes_device(boxes, max_ids=2, any=True)
        with pytest.raises(ValueError):
            c.overlap_boxes_device(boxes, max_ids=0, counts=False)
        with pytest.raises(RtError) as e:
            c.overlap_boxes_device(boxes, cull_mask=0x1FF)
        assert e.value.code == RT_ERR_INVALID_ARGUMENT
        ok()
        # not ready: a stale TLAS after a BLAS refit
        ff, nf = span(sp.geom, 1)
        v = torch.from_numpy(sp.geom.verts[ff:ff + nf].copy()).to("cuda:0")
        torch.cuda.synchronize()
        c.refit_blas_device(1, v)
        err((n, B_, 0xFF, 0, 4, I_, C_), RT_ERR_NOT_READY, "")
        c.set_instances(sp.instances)
        ok()
    finally:
        c.close()
    # trace_variant != 0 (alt library only: the product refuses the parameter itself)
    a = RtContext(0, variant="alt")
    try:
        a.set_param("blas_builder", 0)
        a.set_param("trace_variant", 1)
        a.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        a.set_instances(sp.instances)
        c = a
        err((n, B_, 0xFF, 0, 4, I_, C_), RT_ERR_INVALID_ARGUMENT, "trace_variant 0")
        a.set_param("trace_variant", 0)
        a.set_instances(sp.instances)
        ok()
    finally:
        a.close()
