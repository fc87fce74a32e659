"""The spill half of the traversal stack, for every walk kernel of the product library.

Every walk keeps the first STACK2_LDS = 12 entries of its per-lane stack in LDS and the rest in a per-thread spill area in HBM
("Traversal stack").  The scene here is made of corridors (tests/scenes.py): rows of parallel squares whose trees are
balanced, so that a query along a row holds one entry per level.  A ladder of seven meshes gives modelled peaks of 9 .. 15 entries,
one value each, the deep mesh 17; they stand side by side as instances, with rotated copies whose axes lie along rows of
RT_INSIDE_DIRS, a sheared and mirrored copy, a far-offset one and a long corridor for the shadow rays, under instance masks that a
ray query's own mask byte admits or culls.  Queries aimed at different instances, and at nothing, are
interleaved, so the lanes of a wave sit on both sides of the boundary and refill after short walks.

Every test first asserts its PREMISE with the CPU model of the stack (tests/stack_reference.py) on the context's own snapshot: the
queries it aims at the deep end reach STACK2_LDS + 2 entries or more (frames: + 4), those at the ladder's foot stay in LDS.  Then it
compares the GPU with the tree-independent reference of that family, bit for bit, as the family's own tests do."""
import functools

import numpy as np
import pytest

from tests import closest_reference as cr
from tests import inside_reference as ir
from tests import overlap_reference as orf
from tests import scenes, stack_reference as sr
from tests import sweep_reference as swr
from tests.exact import assert_frame_equals_oracle, assert_hits_equal_oracle
from tests.shade_reference import shade_samples
from tests.test_ray_query_oracle import check_against_oracle, oracle_scene
from vulkan_raytracing_amd import RtContext, api, host, tiling
from vulkan_raytracing_amd.api import INSTANCE_DTYPE

STACK2_LDS = 12                      # the value this file was written for (asserted against kernels.hip below)
SINGLE, FRAME = 2, 4                 # margins of the premises: single-query walks, frames (beams and entry records shift the peak)
LADDER = (256, 512, 1024, 2048, 4096, 8192, 16384)
DEEP = 65536
LIT = 32768                          # the corridor of the shadow test: 14 levels, squares 0.02 apart
MESHES = LADDER + (DEEP, LIT)
DIRS = np.array(api.INSIDE_DIRS, np.float64)
SPACING_X = 48.0
# plane spacings: the deep corridor is 6.6 long instead of 65, so that the rays of a frame's corners, which leave the axis by 0.4 per
# unit, stay inside its footprint to its end and walk all of its levels
SPACING = dict(scenes.CORRIDOR_SPACING)
SPACING[DEEP] = 0.0001
# the shader starts a shadow ray 0.01 off the surface, with tmin 0.001: squares farther apart than that, so that a shadow ray from the
# last square has every other square of the row ahead of it
SPACING[LIT] = 0.02
TERMINATE, CULL_BACK, CULL_FRONT = api.RAY_FLAG_TERMINATE_ON_FIRST_HIT, api.RAY_FLAG_CULL_BACK_FACING, api.RAY_FLAG_CULL_FRONT_FACING


# ---- the scene ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def geometry():
    """(verts, idx, ranges): the ladder meshes and the deep mesh in one pair of buffers"""
    verts, idx, ranges, nf, ni = [], [], [], 0, 0
    for n in MESHES:
        v, ix = scenes.corridor(n, SPACING[n])
        ranges.append((nf, ni, len(ix) // 3))
        verts.append(v.reshape(-1)); idx.append(ix)
        nf += v.size; ni += len(ix)
    return np.concatenate(verts), np.concatenate(idx), ranges


def axis_to(d):
    """a rotation that takes the corridor's axis (0, 0, -1) to the unit vector d"""
    d = np.asarray(d, np.float64) / np.linalg.norm(d)
    u = np.cross(d, (0.0, 1.0, 0.0)); u /= np.linalg.norm(u)
    v = np.cross(u, d)
    return np.stack([u, v, -d], axis=1)              # columns: images of x, y, z; det +1


#            mesh, 3x3, translation
PLACED = [(m, np.eye(3), (SPACING_X * m, 0.0, 0.0)) for m in range(len(LADDER) + 1)] + [
    (6, axis_to(DIRS[0]), (-150.0, 0.0, 0.0)),                                        # 8: the 16384 corridor along RT_INSIDE_DIRS[0]
    (5, axis_to(DIRS[1]), (-150.0, 160.0, 0.0)),                                      # 9: the 8192 corridor along RT_INSIDE_DIRS[1]
    (5, np.array([[1.0, 0.3, 0.0], [0.0, 1.0, 0.0], [0.0, 0.2, -1.0]]), (-260.0, 0.0, 0.0)),   # 10: sheared and mirrored (det -1)
    (6, np.eye(3), (1200.0, 0.0, 0.0)),                                               # 11: far from the rest
    (8, np.eye(3), (-400.0, 0.0, 0.0)),                                               # 12: the lit corridor, 655 long
]
I_DEEP, I_ROT0, I_ROT1, I_SHEAR, I_FAR, I_LIT = 7, 8, 9, 10, 11, 12
# instance masks: every instance is visible to the frames and to a call's cull mask of 0xFF, and a ray query's own mask byte admits some
# of them and culls the others (the walk then pops at the TLAS leaf instead of pushing the marker)
MASKS = (0xFF, 0x01, 0x02, 0x0F, 0xF0, 0x55, 0xAA, 0x3C, 0x0F, 0xF0, 0x81, 0x7E, 0xC3)
# The references of closest points, sweeps, box overlaps and inside tests cost queries x triangles in numpy: a smaller scene of the same
# kind for them, with the ladder's top at 16384 squares (117 000 triangles in all)
SHEAR = np.array([[1.0, 0.3, 0.0], [0.0, 1.0, 0.0], [0.0, 0.2, -1.0]])
PLACED_SMALL = [(m, np.eye(3), (SPACING_X * k, 0.0, 0.0)) for k, m in enumerate((0, 2, 3, 4, 6))] + [
    (6, axis_to(DIRS[0]), (-150.0, 0.0, 0.0)),                                        # 5: along RT_INSIDE_DIRS[0]
    (5, axis_to(DIRS[1]), (-150.0, 160.0, 0.0)),                                      # 6: along RT_INSIDE_DIRS[1]
    (5, SHEAR, (-260.0, 0.0, 0.0)),                                                   # 7: sheared and mirrored
    (3, np.eye(3), (1200.0, 0.0, 0.0)),                                               # 8: far from the rest
]
S_TOP, S_ROT0, S_ROT1, S_SHEAR = 4, 5, 6, 7
SMALL_TARGETS = tuple(range(len(PLACED_SMALL)))
TYPES = [0] * len(PLACED)            # diffuse


def instance_records(placed=PLACED):
    inst = np.zeros(len(placed), INSTANCE_DTYPE)
    for i, (mesh, M, t) in enumerate(placed):
        inst[i] = host.make_instance(np.concatenate([M, np.asarray(t, np.float64)[:, None]], axis=1).astype(np.float32).reshape(12), i, mesh)
        if i % 2 == 1:
            inst[i]["sbt_offset_and_flags"] &= 0x00FFFFFF          # no instance flags: the facing culls of a ray query apply (the others disable them)
        inst[i]["custom_index_and_mask"] = (inst[i]["custom_index_and_mask"] & 0xFFFFFF) | (MASKS[i % len(MASKS)] << 24)
    return inst


def o2w(i, placed=PLACED):
    """the instance's transform as its record holds it (binary32), in binary64"""
    mesh, M, t = placed[i]
    return np.concatenate([M, np.asarray(t, np.float64)[:, None]], axis=1).astype(np.float32).astype(np.float64)


def squares_of(i, placed=PLACED):
    return MESHES[placed[i][0]]


# ---- queries along the corridors ------------------------------------------------------------------------------------------------------

def segments(i, n, rng, placed=PLACED, inside=0.0):
    """n segments along instance i's corridor, world space: from 5 in front of the first square to 5 behind the last one, inside the
    footprint, every other one the other way round; a share `inside` of them starts somewhere within the row.  Returns (from, to,
    whole: the segment runs past both ends)"""
    length = scenes.corridor_length(squares_of(i, placed), SPACING[squares_of(i, placed)])
    a = np.stack([rng.uniform(-7, 7, n), rng.uniform(-7, 7, n), np.full(n, 5.0)], axis=1)
    b = np.stack([rng.uniform(-7, 7, n), rng.uniform(-7, 7, n), np.full(n, -length - 5.0)], axis=1)
    within = rng.uniform(size=n) < inside
    a[within, 2] = -rng.uniform(0.1, 0.9, within.sum()) * length
    swap = np.arange(n) % 2 == 1
    a[swap], b[swap] = b[swap].copy(), a[swap].copy()
    M = o2w(i, placed)
    return a @ M[:, :3].T + M[:, 3], b @ M[:, :3].T + M[:, 3], ~within


def interleave(parts):
    """rows of the parts taken in turn: part k supplies rows k, k + len(parts), ..."""
    n = min(len(p) for p in parts)
    return np.stack([p[:n] for p in parts], axis=1).reshape(n * len(parts), -1)


def corridor_rays(targets, per, seed, placed=PLACED, inside=0.25, misses=True):
    """(rays8, target of every ray or -1, target of every ray that runs the whole length of its corridor or -2): rays along the
    corridors of `targets` and rays that meet nothing, interleaved"""
    rng = np.random.default_rng(seed)
    parts, tag, whole = [], [], []
    for i in targets:
        a, b, w = segments(i, per, rng, placed, inside)
        whole.append(np.where(w, i, -2))
        d = (b - a) / np.linalg.norm(b - a, axis=1, keepdims=True)
        r = np.zeros((per, 8))
        r[:, 0:3] = a; r[:, 3] = 0.001; r[:, 4:7] = d; r[:, 7] = 10000.0
        parts.append(r); tag.append(np.full(per, i))
    if misses:
        r = np.zeros((per, 8))
        r[:, 0:3] = rng.uniform(-50, 50, (per, 3)) + (0.0, 600.0, 0.0); r[:, 3] = 0.001; r[:, 5] = 1.0; r[:, 7] = 10000.0
        parts.append(r); tag.append(np.full(per, -1)); whole.append(np.full(per, -1))
    return interleave(parts).astype(np.float32), interleave([t[:, None] for t in tag]).reshape(-1), interleave([t[:, None] for t in whole]).reshape(-1)


ALL_TARGETS = tuple(range(len(PLACED)))


def premise(model, queries, tags, deep, shallow=(0,), margin=SINGLE, sample=6, what=""):
    """The premise of a test: of the queries aimed at each instance of `deep`, a sample reaches STACK2_LDS + margin entries before
    the first triangle is tested (a lower bound of the kernel's peak); those aimed at `shallow` stay in the LDS part in a walk that
    prunes nothing (an upper bound).  Returns {instance: (lowest, highest) modelled peak of the sample}."""
    assert sr.stack2_lds() == STACK2_LDS
    peaks = {}
    for i in tuple(deep) + tuple(shallow):
        sel = np.nonzero(np.asarray(tags) == i)[0][:sample]
        assert len(sel) >= min(sample, 2), (what, i)
        if i in deep:
            p = [model.first(queries[k]) for k in sel]
            assert min(p) >= STACK2_LDS + margin, "%s: the queries at instance %d peak at %s, not in the spill area" % (what, i, p)
        else:
            p = [model.full(queries[k]) for k in sel]
            assert max(p) < STACK2_LDS, "%s: the queries at instance %d peak at %s, not inside LDS" % (what, i, p)
        peaks[i] = (min(p), max(p))
    print("%s: modelled peaks %s" % (what, peaks))
    return peaks


# ---- CPU: the scene's premise on host-built trees ------------------------------------------------------------------------------------

def host_model(placed):
    v, ix, ranges = geometry()
    meshes = []
    for mesh, M, t in placed:
        ff, fi, pc = ranges[mesh]
        nv = int(ix[fi:fi + 3 * pc].max()) + 1
        meshes.append((v[ff:ff + 6 * nv].reshape(-1, 6), ix[fi:fi + 3 * pc]))
    return sr.StackModel(sr.host_snapshot(meshes, [o2w(i, placed).reshape(12) for i in range(len(placed))]))


def test_the_scene_spans_the_boundary_on_host_built_trees():
    """without a GPU: the instances' modelled peaks over host-built trees under a balanced TLAS.  The ladder instances take every
    value from STACK2_LDS - 3 to STACK2_LDS + 3, the deep one STACK2_LDS + 5, and the transformed copies spill by the margin."""
    model = host_model(PLACED)
    rays, tag, _ = corridor_rays(ALL_TARGETS, 4, seed=1, inside=0.0)
    q = sr.rays_of(rays)
    peaks = {i: sorted({model.first(q[k]) for k in np.nonzero(tag == i)[0]}) for i in ALL_TARGETS}
    for i in ALL_TARGETS:                                # the BLAS part is the tree's depth; the TLAS adds its pending siblings
        levels = int(np.log2(squares_of(i))) - 1
        assert {model.peak(q[k], blas_only=i)[0] for k in np.nonzero(tag == i)[0]} == {levels}, i
        assert levels + 2 <= peaks[i][0] and peaks[i][-1] <= levels + 2 + 4, (i, peaks[i])
    # sentinel + marker + one entry per level: the ladder's own part of the peak, STACK2_LDS - 3 .. STACK2_LDS + 3.  The balanced TLAS
    # of this CPU snapshot keeps one sibling pending for most rays, for every ray at the ladder's top: the full peaks seen here are
    # sure to take the values up to STACK2_LDS + 2 and may skip STACK2_LDS + 3 (the context's own TLAS is modelled in every GPU test)
    assert [int(np.log2(n)) - 1 + 2 for n in LADDER] == list(range(STACK2_LDS - 3, STACK2_LDS + 4))
    assert set(range(STACK2_LDS - 3, STACK2_LDS + 3)) <= set().union(*(peaks[i] for i in range(len(LADDER)))), peaks
    assert min(peaks[0]) < STACK2_LDS - 2 and peaks[I_DEEP][0] >= STACK2_LDS + 5
    assert all(peaks[i][0] >= STACK2_LDS + SINGLE for i in (I_ROT0, I_ROT1, I_SHEAR, I_FAR, I_LIT)), peaks
    assert {model.full(q[k]) for k in np.nonzero(tag == -1)[0]} == {1}


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

class World:
    """one context over the scene (host-built trees), its snapshot's model, the oracle and the numpy scene of the references"""

    def __init__(self, builder="host", mp=None, placed=PLACED, device_tlas=False):
        from tests.test_ray_query import dev_inst
        from tests.test_ray_query_hits import hits_scene
        from tests.test_ray_query_oracle import use_builder
        self.placed = placed
        self.verts, self.idx, self.ranges = geometry()
        self.inst = instance_records(placed)
        self.ctx = RtContext(0)
        try:
            if mp is None:
                self.ctx.set_param("blas_builder", 0)
            else:
                use_builder(self.ctx, builder, mp)
            self.ctx.upload_geometry(self.verts, self.idx, self.ranges)
            if device_tlas:
                self.ctx.set_instances_device(dev_inst(self.inst))
                self.ctx.synchronize()
            else:
                self.ctx.set_instances(self.inst)
            self.model = sr.StackModel(self.ctx.debug_snapshot())
        except BaseException:
            self.ctx.close()
            raise
        self.orc = hits_scene(self.verts, self.idx, self.ranges, self.inst)
        self._sc = self._tris = None

    @property
    def sc(self):
        if self._sc is None:
            self._sc = cr.Scene(self.verts, self.idx, self.ranges, self.inst)
        return self._sc

    @property
    def tris(self):
        if self._tris is None:
            self._tris = orf.Triangles(self.sc)
        return self._tris


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.ctx.close()


def dev(a, cols=8):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1, cols).copy()).to("cuda:0")


def dev_words(w):
    import torch
    return torch.from_numpy(np.ascontiguousarray(w, np.uint32).view(np.int32).copy()).to("cuda:0")


SPILLING = (6, I_DEEP, I_ROT0, I_ROT1, I_SHEAR, I_FAR, I_LIT)      # modelled peaks of STACK2_LDS + 2 and more on host-built trees


def check_first_hits(orc, rays, h, words=None):
    """any-hit records: hit or miss as the closest hit says, and every hit a candidate the oracle accepts with these very fields"""
    ref = orc.intersect(rays)
    assert np.array_equal(h["inst"] >= 0, ref["inst"] >= 0)
    fh = np.nonzero(h["inst"] >= 0)[0]
    ok, c, _ = orc.query_candidate(rays[fh], h["inst"][fh], h["prim"][fh], None if words is None else words[fh], 0, 0xFF)
    assert ok.all() and c.tobytes() == h[fh].tobytes()
    miss = h["inst"] < 0
    assert h[miss].tobytes() == ref[miss].tobytes()


@pytest.mark.gpu
def test_closest_and_any_hit_rays(world):
    """k_trace's query instantiations (rt_intersect_device): 1001 rays down and up every corridor and past all of them, interleaved"""
    import torch
    rays, tag, whole = corridor_rays(ALL_TARGETS, 77, seed=11)
    assert len(rays) % 64 != 0
    premise(world.model, sr.rays_of(rays), whole, SPILLING, what="ray queries")
    closest = world.ctx.intersect_device(dev(rays), attributes=True)
    first = world.ctx.intersect_device(dev(rays), any_hit=True)
    torch.cuda.synchronize()
    h, a = closest.numpy()
    ref = assert_hits_equal_oracle(h, world.orc, rays)
    bf = world.orc.intersect(rays[::7], use_bvh=False)
    assert h[::7].tobytes() == bf.tobytes()
    assert set(np.unique(ref["inst"])) == set(ALL_TARGETS) | {-1}
    o = world.orc.hit_attributes(h)
    assert np.array_equal(a.view(np.float32)[:, 0:3].view(np.uint32), o[:, 0:3].view(np.uint32))
    check_first_hits(world.orc, rays, first.numpy()[0])


def flag_words(n, seed):
    """per-ray words: facing culls (the squares face +z: a cull leaves a ray nothing and it walks the whole row), TerminateOnFirstHit
    mixed in, a cull mask byte of its own per ray: it admits some of the instances (MASKS) and culls the others"""
    rng = np.random.default_rng(seed)
    w = rng.choice([0, CULL_BACK, CULL_FRONT, TERMINATE, TERMINATE | CULL_BACK, TERMINATE | CULL_FRONT], n).astype(np.uint32)
    mask = np.where(rng.uniform(size=n) < 0.6, 1 << rng.integers(0, 8, n), rng.integers(1, 256, n))      # single bits cull about half the instances
    w |= (mask.astype(np.uint32) << 24)
    w[::9] = 0xFF000000
    return w


@pytest.mark.gpu
def test_ray_flags_and_cull_masks(world):
    """k_trace's flags instantiation (rt_intersect_device_flags): per-ray words against the oracle"""
    import torch
    rays, tag, whole = corridor_rays(ALL_TARGETS, 77, seed=12)
    premise(world.model, sr.rays_of(rays), whole, SPILLING, what="ray flags")
    words = flag_words(len(rays), 13)
    res = world.ctx.intersect_device_flags(dev(rays), words=dev_words(words), attributes=True)
    torch.cuda.synchronize()
    h, a = res.numpy()
    check_against_oracle(world.orc, rays, words, 0, 0xFF, h, a, what="corridors")
    cull = ((words & (CULL_BACK | CULL_FRONT)) != 0) & np.isin(whole, SPILLING)     # every square faces the same way: such a ray hits the first one or none
    assert (h["inst"][cull] == -1).sum() > 5 and (h["inst"][cull] >= 0).sum() > 5
    for i in (6, I_DEEP, I_LIT):                      # mask culls: rays along a spilling corridor that enter it, and rays that must skip it
        aimed = (whole == i) & ((words & (CULL_BACK | CULL_FRONT)) == 0)
        admitted = ((words >> 24) & MASKS[i]) != 0
        assert (aimed & admitted).sum() > 3 and (aimed & ~admitted).sum() > 3, i
        assert (h["inst"][aimed & admitted] == i).all() and (h["inst"][aimed & ~admitted] != i).all(), i
    res = world.ctx.intersect_device_flags(dev(rays), ray_flags=TERMINATE, attributes=True)
    torch.cuda.synchronize()
    h, a = res.numpy()
    check_against_oracle(world.orc, rays, None, TERMINATE, 0xFF, h, a, what="corridors, first hits")


@pytest.mark.gpu
def test_hit_lists_and_counts(world):
    """k_query_hits (rt_intersect_device_hits): max_hits 1, 16 and 0, with and without counts.  A count-only walk prunes nothing:
    its modelled full peak is exact."""
    from tests.test_ray_query_hits import check_lists, gpu_hits, oracle_lists, truncate
    rays, tag, whole = corridor_rays(ALL_TARGETS, 6, seed=14, inside=0.1)
    assert len(rays) == 84
    premise(world.model, sr.rays_of(rays), whole, SPILLING, sample=3, what="hit lists")
    words = flag_words(len(rays), 15) & ~np.uint32(TERMINATE)
    for w in (None, words):
        ref = oracle_lists(world.orc, rays, w, 0, 0xFF, 16)
        assert ref[2].max() >= MESHES[-1] // 2 and (ref[2] == 0).sum() >= 6
        for K in (16, 1):
            check_lists(world.orc, gpu_hits(world.ctx, rays, w, 0, 0xFF, K, attributes=K == 16), truncate(ref, K), "K %d" % K)
            h, _, c = gpu_hits(world.ctx, rays, w, 0, 0xFF, K, counts=False)
            assert c is None and h.tobytes() == truncate(ref, K)[0].tobytes()
        h, _, c = gpu_hits(world.ctx, rays, w, 0, 0xFF, 0)
        assert h is None and np.array_equal(c, ref[2])


@pytest.fixture(scope="module")
def small():
    w = World(placed=PLACED_SMALL)
    yield w
    w.ctx.close()


_CLOSEST = {}


def closest_points_and_reference(small):
    """(points4, target of every point, brute32's records), computed once: points 3 in front of and behind the corridors of the small
    scene (the search descends towards the near end and keeps the far half of every level), some with a radius that ends inside the
    row, and points far away with a radius that reaches nothing"""
    if not _CLOSEST:
        rays, tag, _ = corridor_rays(SMALL_TARGETS, 4, seed=16, placed=PLACED_SMALL, inside=0.0)
        pts = np.zeros((len(rays), 4), np.float32)
        pts[:, 0:3] = rays[:, 0:3] + np.float32(2.0) * rays[:, 4:7]        # 3 off an end of the row, inside the footprint
        pts[:, 3] = np.where(np.arange(len(pts)) % 7 == 6, 4.0, np.inf)
        pts[tag == -1, 3] = 5.0
        pts[tag == 0, 3] = 6.0    # (the shallow end: a radius bounds the walk, so that the model's unpruned walk bounds it too)
        _CLOSEST["x"] = (pts, tag, cr.brute32(small.sc, pts))
    return _CLOSEST["x"]


def closest_premise(small, pts, tag):
    q = [sr.Point(p[0:3], p[3]) for p in pts.astype(np.float64)]
    premise(small.model, q, np.where(np.isinf(pts[:, 3]) | (tag == 0), tag, -2), (S_TOP, S_ROT0, S_ROT1, S_SHEAR), sample=3, what="closest points")


@pytest.mark.gpu
def test_closest_points(small):
    """k_closest_point against the binary32 brute force, byte for byte"""
    import torch
    pts, tag, ref = closest_points_and_reference(small)
    closest_premise(small, pts, tag)
    res = small.ctx.closest_point_device(dev(pts, 4), attributes=True)
    torch.cuda.synchronize()
    h, a = res.numpy()
    assert h.tobytes() == ref.tobytes(), np.nonzero(h != ref)[0][:5]
    assert (ref["inst"][tag == -1] == -1).all() and (ref["inst"][tag >= 0] == tag[tag >= 0]).all()
    kinds, _ = cr.side_words(small.sc, pts, ref)
    assert np.array_equal(a[:, 7].view(np.uint32), kinds)


@pytest.mark.gpu
def test_sphere_sweeps(small):
    """k_sweep_spheres: r = 0 and r > 0 along the corridors"""
    import torch
    rays, tag, whole = corridor_rays(SMALL_TARGETS, 8, seed=17, placed=PLACED_SMALL)
    s = rays.copy()
    s[:, 3] = np.where(np.arange(len(s)) % 4 < 2, 0.0, 0.35)
    s[:, 7] = np.where(np.arange(len(s)) % 7 == 6, 30.0, 200.0)
    premise(small.model, sr.rays_of(s, r=True), np.where(s[:, 7] > 100.0, whole, -2), (S_TOP, S_ROT0), sample=3, what="sphere sweeps")
    res = small.ctx.sweep_spheres_device(dev(s), attributes=False)
    torch.cuda.synchronize()
    h = res.numpy()[0]
    ref = swr.brute32(small.sc, s, pairs=swr.candidate_pairs(small.sc, s))
    assert h.tobytes() == ref.tobytes(), np.nonzero(h != ref)[0][:5]
    assert (ref["inst"][tag == -1] == -1).all() and (ref["inst"][tag >= 0] >= 0).mean() > 0.9


def corridor_boxes(targets, per, seed):
    """boxes that cover a whole corridor and boxes around a stretch of it (world-space bounds of a segment along the row, widened),
    interleaved with boxes that touch nothing.  Returns (boxes8, target or -1, target of the boxes that cover their corridor or -2)"""
    rng = np.random.default_rng(seed)
    parts, tag, whole = [], [], []
    for i in targets:
        a, b, _ = segments(i, per, rng, PLACED_SMALL, inside=0.0)
        part = rng.uniform(0.3, 0.6, (per, 1)) * (np.arange(per) % 3 == 1)[:, None]         # every third box: a stretch from one end
        whole.append(np.where(part[:, 0] > 0, -2, i))
        b = np.where(part > 0, a + (b - a) * part, b)
        pad = np.where(np.arange(per)[:, None] % 4 < 2, 12.0, 0.5)
        box = np.zeros((per, 8))
        box[:, 0:3] = np.minimum(a, b) - pad; box[:, 4:7] = np.maximum(a, b) + pad
        parts.append(box); tag.append(np.full(per, i))
    box = np.zeros((per, 8))
    box[:, 0:3] = rng.uniform(-50, 50, (per, 3)) + (0.0, 600.0, 0.0); box[:, 4:7] = box[:, 0:3] + 3.0
    parts.append(box); tag.append(np.full(per, -1)); whole.append(np.full(per, -1))
    return interleave(parts).astype(np.float32), interleave([t[:, None] for t in tag]).reshape(-1), interleave([t[:, None] for t in whole]).reshape(-1)


@pytest.mark.gpu
def test_box_overlaps(small):
    """k_overlap_boxes: ids, counts and RT_OVERLAP_ANY.  The walk prunes nothing when it counts: the modelled full peak is exact."""
    import torch
    boxes, tag, whole = corridor_boxes(SMALL_TARGETS, 8, seed=18)
    q = [sr.Box(b[0:3], b[4:7]) for b in boxes.astype(np.float64)]
    premise(small.model, q, whole, (S_TOP, S_ROT0, S_ROT1, S_SHEAR), sample=3, what="box overlaps")
    rc, ri = orf.brute32(small.sc, boxes, tris=small.tris)
    assert rc.max() >= 2 * 16384 and (rc[tag == -1] == 0).all() and (rc[tag >= 0] > 0).all()

    def run(**kw):
        res = small.ctx.overlap_boxes_device(dev(boxes), **kw)
        torch.cuda.synchronize()
        return res.numpy()

    counts, ids = run(max_ids=16)
    assert counts.tobytes() == rc.tobytes() and ids.tobytes() == ri.tobytes()
    counts, ids = run(max_ids=3, counts=False)
    assert counts is None and ids.tobytes() == np.ascontiguousarray(ri[:, :3]).tobytes()
    counts, ids = run(max_ids=0)
    assert ids is None and counts.tobytes() == rc.tobytes()
    occ, ids = run(max_ids=0, any=True)
    assert ids is None and np.array_equal(occ, (rc > 0).astype(np.uint32))


@pytest.mark.gpu
def test_points_inside_and_signed_distance(small):
    """k_point_inside: the rays of RT_INSIDE_DIRS from points at the ends of the rotated corridors, whose axes lie along rows 0 and 1
    of the table: the first (second) direction runs down the whole row.  An inside walk counts every crossing and prunes nothing."""
    import torch
    rng = np.random.default_rng(19)
    parts, tags = [], []
    for i, k in ((S_ROT0, 0), (S_ROT1, 1)):
        a, b, _ = segments(i, 16, rng, PLACED_SMALL)
        a[1::2] = b[1::2] - (b[1::2] - a[1::2]) * rng.uniform(0.0, 0.5, (8, 1))           # (odd segments start behind the row: points within it instead)
        parts.append(a); tags.append(np.full(16, i))
    a, _, _ = segments(0, 16, rng, PLACED_SMALL)
    parts.append(a); tags.append(np.full(16, 0))
    parts.append(rng.uniform(-50, 50, (16, 3)) + (0.0, 600.0, 0.0)); tags.append(np.full(16, -1))
    p3, tag = interleave(parts), interleave([t[:, None] for t in tags]).reshape(-1)
    pts = np.concatenate([p3, np.full((len(p3), 1), np.inf)], axis=1).astype(np.float32)
    rays = ir.compose_rays(pts, 5)
    q = sr.rays_of(rays)
    for i, k in ((S_ROT0, 0), (S_ROT1, 1)):
        peaks = [small.model.first(q[5 * j + k]) for j in np.nonzero(tag == i)[0][:6:2]]            # (points in front of the row)
        assert min(peaks) >= STACK2_LDS + SINGLE, (i, peaks)
        print("inside: instance %d, direction %d: modelled peaks %s" % (i, k, peaks))
    ref = ir.oracle_counts(small.orc, small.orc.tri_counts, pts, 5)
    assert ref[tag == S_ROT0, 0].max() > 10000 and (ref[tag == -1] == 0).all()
    for n_dirs in (1, 3, 5):
        for counts in (True, False):
            res = small.ctx.point_inside_device(dev(pts, 4), n_dirs=n_dirs, counts=counts)
            torch.cuda.synchronize()
            w, c = res.numpy()
            if counts:
                assert np.array_equal(c, ref[:, :n_dirs]), n_dirs
            else:
                assert c is None
            assert np.array_equal(w, ir.words(ref, n_dirs, counts)), (n_dirs, counts)
    cp = small.ctx.closest_point_device(dev(pts, 4))
    sd = small.ctx.signed_distance_device(dev(pts, 4), n_dirs=3)
    torch.cuda.synchronize()
    ch, sh = cp.numpy()[0], sd.numpy()[0]
    inside = (ir.words(ref, 3, False) & 1).astype(bool)
    want = ch.copy()
    want["t"] = np.where(inside, -ch["t"], ch["t"])
    assert sh.tobytes() == want.tobytes()
    assert ch.tobytes() == cr.brute32(small.sc, pts).tobytes()


@pytest.mark.gpu
def test_more_rays_than_the_resident_grid_has_threads(world, small):
    """More records than the resident grid has threads: 1 078 distinct rays, and the 40 points of test_closest_points, repeated.  Every
    wave that starts takes chunks of 64 of them, each chunk with queries on both sides of the boundary, so every thread of the resident
    grid uses its own spill row.  Every record is held to the reference of the query it repeats."""
    import torch
    rays, tag, whole = corridor_rays(ALL_TARGETS, 77, seed=21)
    premise(world.model, sr.rays_of(rays), whole, SPILLING, what="a full grid of rays")
    reps = 256 * 8 * 256 // len(rays) + 2
    many = np.tile(rays, (reps, 1))
    assert len(many) > 256 * 8 * 256 and len(many) % 64 != 0       # (MI355X: 256 CUs, at most 8 resident workgroups of 256 threads each)
    ref = world.orc.intersect(rays)
    res = world.ctx.intersect_device(dev(many))
    torch.cuda.synchronize()
    h = res.numpy()[0]
    assert h.tobytes() == np.tile(ref, reps).tobytes()
    pts, tag, cref = closest_points_and_reference(small)
    closest_premise(small, pts, tag)
    reps = 256 * 8 * 256 // len(pts) + 3
    many = np.tile(pts, (reps, 1))
    assert len(many) > 256 * 8 * 256 and len(many) % 64 != 0
    res = small.ctx.closest_point_device(dev(many, 4))
    torch.cuda.synchronize()
    assert res.numpy()[0].tobytes() == np.tile(cref, reps).tobytes()


# ---- shading: caller rays, frames, shadow rays -----------------------------------------------------------------------------------------

FW, FH, SPP, BOUNCES = 92, 60, 2, 3            # a small frame, no multiple of the 8 x 8 tile
GLASS = [2 if i == I_DEEP else (1 if i == 6 else 0) for i in range(len(PLACED))]     # a refractive deep corridor, a mirror one, diffuse


def frame_uniforms(position, light=(SPACING_X * I_DEEP + 1.0, 3.0, 12.0), bounces=BOUNCES, spp=SPP):
    u = host.default_uniforms(max_bounce_count=bounces, samples_per_pixel=spp, center_object_type=0, orbiting_object_type=0,
                              orbiting_object_primitive_offset=0, orbiting_object_vertex_offset=0)
    u[0]["position"][:3] = position          # (the default camera looks along -z: down the corridors)
    u[0]["light_position"][:3] = light
    return u


IN_FRONT = (SPACING_X * I_DEEP, 0.0, 6.0)     # the deep corridor's first square fills the view


def shading_scene(w, types, u):
    """the same uniforms, instance types and sky on the context and the oracle"""
    sky = scenes.synthetic_skybox(32)
    for t in (w.ctx, w.orc):
        t.set_instance_types(types)
        t.set_skybox(sky)
    w.ctx.set_uniforms(u)
    w.orc.set_uniforms(u.tobytes())


def centre_rays(orc, W, H, step=9):
    """the primary ray of sample 0 of every step-th pixel, as query rays"""
    xy = [(x, y) for y in range(0, H, step) for x in range(0, W, step)] + [(W - 1, H - 1)]
    r = np.zeros((len(xy), 8), np.float32)
    for k, (x, y) in enumerate(xy):
        od = orc.primary_ray(x, y, W, H, 0)
        r[k] = (od[0], od[1], od[2], 0.001, od[3], od[4], od[5], 10000.0)
    return r


def frame_premise(w, what, margin=FRAME):
    """every sampled primary ray, walked from the TLAS root, holds STACK2_LDS + margin entries before its first triangle"""
    assert sr.stack2_lds() == STACK2_LDS
    rays = centre_rays(w.orc, FW, FH)
    assert (w.orc.intersect(rays, use_bvh=False)["inst"] == I_DEEP).all(), "the deep corridor fills the view"
    peaks = [w.model.first(q) for q in sr.rays_of(rays)]
    assert min(peaks) >= STACK2_LDS + margin, (what, peaks)
    print("%s: modelled peaks of %d primary rays: %d .. %d" % (what, len(peaks), min(peaks), max(peaks)))


def counts(st):
    return (int(st.rays_primary), int(st.rays_secondary), int(st.rays_shadow))


_RENDERS = {}


def oracle_frame(w, types, u):
    """the oracle's frame and ray counts for these types and uniforms, rendered once (w.orc must be in that state)"""
    key = (tuple(types), u.tobytes())
    if key not in _RENDERS:
        _RENDERS[key] = w.orc.render(FW, FH)
    return _RENDERS[key]


DEFAULTS = {"fused_shade": 1, "camera_records": 1, "pixel_beams": 1, "tail_kernel": 1}


@pytest.fixture
def frames(world):
    """the world's context for frames; whatever a test sets is set back"""
    yield world
    for k, v in DEFAULTS.items():
        world.ctx.set_param(k, v)
    world.ctx.set_instances(world.inst)
    world.ctx.set_instance_types([0] * len(PLACED))
    world.orc.set_instance_types([0] * len(PLACED))


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["default", "fused_shade=0", "camera_records=0", "pixel_beams=0", "tail_kernel=0", "tail_kernel=2"])
def test_frames_down_the_deep_corridor(frames, setting):
    """k_beam_shade (default), k_beam + k_shade (fused_shade 0), the walk from the TLAS root (camera_records 0), one walk per ray
    (pixel_beams 0), the late bounces in k_trace or k_tail: the camera looks down the deep corridor, whose front plane refracts, so
    the secondary rays go on down the row from inside it, three bounces deep"""
    w = frames
    shading_scene(w, GLASS, frame_uniforms(IN_FRONT))
    frame_premise(w, "frame, " + setting)
    if setting != "default":
        name, value = setting.split("=")
        w.ctx.set_param(name, int(value))
    ref, rc = oracle_frame(w, GLASS, frame_uniforms(IN_FRONT))
    assert rc[0] == FW * FH * SPP and rc[1] == BOUNCES * rc[0]           # every sample goes on through the glass, bounce after bounce
    img, st = w.ctx.trace(FW, FH)
    assert_frame_equals_oracle(img, w.orc, FW, FH, ref=ref)
    assert counts(st) == tuple(int(x) for x in rc)


@pytest.mark.gpu
def test_frame_batch_slot_and_shards(frames):
    """a batch of two frames (their own cameras), a second frame slot rendering beside the root, and a 3-shard split reassembled"""
    import torch
    w = frames
    u0, u1 = frame_uniforms(IN_FRONT), frame_uniforms((IN_FRONT[0] + 0.5, -0.25, 5.0))
    refs = []
    for u in (u0, u1):
        shading_scene(w, GLASS, u)
        frame_premise(w, "batch frame")
        refs.append(oracle_frame(w, GLASS, u))
    # the batch
    w.ctx.set_batch(np.stack([w.inst, w.inst]), np.concatenate([u0, u1]))
    buf = torch.zeros((2, FH, FW, 4), dtype=torch.float32, device="cuda:0")
    w.ctx.trace_shard_batch(FW, FH, 8, 0, 1, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream, frame_stride_bytes=FH * FW * 16)
    st = w.ctx.stats()
    out = buf.cpu().numpy()
    w.ctx.set_instances(w.inst)
    for k, u in enumerate((u0, u1)):
        w.orc.set_uniforms(u.tobytes())
        assert_frame_equals_oracle(out[k], w.orc, FW, FH, ref=refs[k][0])
    assert counts(st) == tuple(int(a) + int(b) for a, b in zip(refs[0][1], refs[1][1]))
    # a second slot beside the root
    w.ctx.set_uniforms(u1)
    slot = w.ctx.frame_slot()
    try:
        slot.set_instance_types(GLASS)
        slot.set_instances(w.inst)
        slot.set_uniforms(u0)
        slot.trace_async(FW, FH)
        img1, st1 = w.ctx.trace(FW, FH)
        img0, st0 = slot.trace_wait()
    finally:
        slot.close()
    assert_frame_equals_oracle(img1, w.orc, FW, FH, ref=refs[1][0])
    w.orc.set_uniforms(u0.tobytes())
    assert_frame_equals_oracle(img0, w.orc, FW, FH, ref=refs[0][0])
    assert counts(st0) == tuple(int(x) for x in refs[0][1]) and counts(st1) == tuple(int(x) for x in refs[1][1])
    # three shards
    w.ctx.set_uniforms(u0)
    rows = tiling.max_shard_rows(FH, 8, 3)
    shards, total = [], np.zeros(3, np.int64)
    for s in range(3):
        buf = torch.zeros((rows, FW, 4), dtype=torch.float32, device="cuda:0")
        w.ctx.trace_shard(FW, FH, 8, s, 3, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
        w.ctx.synchronize()
        total += counts(w.ctx.stats())
        shards.append(buf.cpu().numpy())
    assert_frame_equals_oracle(tiling.assemble(shards, FH, FW, 8), w.orc, FW, FH, ref=refs[0][0])
    assert tuple(total) == tuple(int(x) for x in refs[0][1])


def replay_first_bounce(orc, rays):
    """the oracle's own first bounce of the given primary rays: (hits, shadow rays as query rays, index of their primary ray)"""
    hits = orc.intersect(rays)
    st = orc.bounce_step(np.concatenate([rays[:, 0:3], rays[:, 4:7]], axis=1), np.zeros(len(rays), np.uint32), hits)
    sh = np.nonzero(st[:, 0].astype(np.int32) == 2)[0]
    s8 = np.zeros((len(sh), 8), np.float32)
    s8[:, 0:3] = st[sh, 8:11]; s8[:, 3] = 0.001; s8[:, 4:7] = st[sh, 11:14]; s8[:, 7] = st[sh, 14]
    return hits, s8, sh


def shadow_setup(w):
    """The shadow walk.  A shadow ray that runs along a corridor needs a lit surface inside it: the camera stands at the far end of the
    lit corridor (32768 squares, 0.02 apart), between its last two squares, and looks at the last one (diffuse, facing it); the light
    stands in front of the corridor's first square.  The shader starts the shadow ray 0.01 off the surface, before the last square
    but one, so it has 32767 squares ahead of it and enters both children at every one of the 14 levels.  (The primary rays have one
    square ahead of them: they are not what this frame is about.)"""
    x = PLACED[I_LIT][2][0]
    u = frame_uniforms((x, 0.0, -(LIT - 1.5) * SPACING[LIT]), light=(x + 0.5, 0.3, 12.0), bounces=1)
    shading_scene(w, [0] * len(PLACED), u)
    return u


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["default", "fused_shade=0"])
def test_shadow_rays_up_a_corridor(frames, setting):
    """The shadow instantiation of trace_body (any hit, started from the light's entry records; the product library has no shadow
    beams).  The oracle's own first bounce gives the shadow rays whose walk the model measures from the TLAS root; an entry record
    can start the walk inside the tree with up to ENTRY_WORDS words in another order, so the premise takes the frames' margin.  The
    oracle counts one shadow ray per sample, and the library's rays_shadow_untraced says that it walked them all."""
    w = frames
    u = shadow_setup(w)
    assert sr.stack2_lds() == STACK2_LDS
    rays = centre_rays(w.orc, FW, FH)
    hits, shadow, src = replay_first_bounce(w.orc, rays)
    assert len(src) == len(rays) and (hits["inst"] == I_LIT).all(), "every primary ray ends on the lit square and casts a shadow ray"
    assert (w.orc.intersect(shadow, any_hit=True)["inst"] == I_LIT).all()
    peaks = [w.model.first(q) for q in sr.rays_of(shadow)]
    assert min(peaks) >= STACK2_LDS + FRAME, peaks
    print("shadow rays, %s: modelled peaks %d .. %d" % (setting, min(peaks), max(peaks)))
    if setting != "default":
        name, value = setting.split("=")
        w.ctx.set_param(name, int(value))
    ref, rc = oracle_frame(w, [0] * len(PLACED), u)
    img, st = w.ctx.trace(FW, FH)
    assert_frame_equals_oracle(img, w.orc, FW, FH, ref=ref)
    assert counts(st) == tuple(int(x) for x in rc) and rc[2] == FW * FH * SPP      # a live shadow ray per sample: all of them
    assert int(st.rays_shadow_untraced) == 0, "every shadow ray of the frame is walked"


@pytest.mark.gpu
def test_caller_rays_down_the_corridors(frames):
    """rt_shade_rays_device: caller rays down a refractive, a mirror and diffuse corridors, interleaved with rays into the sky"""
    import torch
    w = frames
    shading_scene(w, GLASS, frame_uniforms(IN_FRONT))
    rays, tag, whole = corridor_rays((0, 3, 6, I_DEEP, I_ROT0, I_SHEAR), 43, seed=31)
    assert len(rays) == 301
    premise(w.model, sr.rays_of(rays), whole, (6, I_DEEP, I_ROT0, I_SHEAR), what="caller rays")
    n_points = len(rays)
    records = np.concatenate([rays, rays])                                # two samples per point
    want = shade_samples(w.orc, records, n_points, BOUNCES)
    s, p = w.ctx.shade_rays_device(dev(records), samples=2)
    torch.cuda.synchronize()
    s, p = s.cpu().numpy(), p.cpu().numpy()
    assert np.array_equal(s.view(np.uint32), want.view(np.uint32)), np.nonzero((s != want).any(axis=1))[0][:8]
    from tests.shade_reference import average_points
    assert np.array_equal(p.view(np.uint32), average_points(want, n_points, 2).view(np.uint32))
    assert len(np.unique(want[:, :3], axis=0)) > 20


# ---- spill areas that must regrow; device-built trees ---------------------------------------------------------------------------------

def deep_mesh_arrays(n=96, s=0.5):
    """test_launch_tunables.deep_mesh as arrays: triangles facing +z about the z axis, each half the size of the one before and
    nearer the origin; the host builder's tree over them has 40 levels, more than the smallest spill area holds"""
    a = 4.0 * s ** np.arange(n)
    v = np.zeros((n, 3, 6), np.float32)
    v[:, 0, 0:3] = np.stack([-a, -a, -a], axis=1)
    v[:, 1, 0:3] = np.stack([3.0 * a, -a, -a], axis=1)
    v[:, 2, 0:3] = np.stack([-a, 3.0 * a, -a], axis=1)
    v[:, :, 5] = 1.0
    return v.reshape(-1), np.arange(3 * n, dtype=np.uint32), [(0, 0, n)]


@pytest.mark.gpu
def test_spill_areas_regrow_when_the_trees_get_deeper():
    """One context: a frame and a query on a shallow scene (the teapot: the smallest spill stride), then a 40-level tree (a wider
    stride: the frame's area and the query workspace's area are both reallocated, on different paths), then the shallow scene again.
    The queries walk the 40-level mesh along its axis; the frame looks down the deep corridor, which stands beside it."""
    import os
    import torch
    from tests.test_launch_tunables import axis_rays
    v, ix, ranges = deep_mesh_arrays()
    rc, info = api.check_builders(v, ix)
    assert rc == 0 and info["depth"] >= 40, info
    cv, ci = scenes.corridor(DEEP, SPACING[DEEP])
    ranges = ranges + [(len(v), len(ix), len(ci) // 3)]
    v, ix = np.concatenate([v, cv.reshape(-1)]), np.concatenate([ix, ci])
    ident = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    aside = np.array([1, 0, 0, 100.0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    inst = np.asarray([host.make_instance(ident, 0, 0), host.make_instance(aside, 1, 1)], INSTANCE_DTYPE)
    u = frame_uniforms((100.0, 0.0, 6.0), light=(101.0, 3.0, 12.0), bounces=1)
    deep_orc = oracle_scene(v, ix, ranges, inst)
    deep_orc.set_uniforms(u.tobytes())
    deep_orc.set_skybox(scenes.synthetic_skybox(32))
    deep_ref, deep_rc = deep_orc.render(FW, FH)
    rays = axis_rays(4096 + 17, seed=5)
    deep_hits = deep_orc.intersect(rays, use_bvh=False)
    assert (deep_hits["inst"] == 0).all()
    teapot_rays = scenes.random_rays(4096 + 17, seed=6)
    c = RtContext(0)
    try:
        c.set_param("blas_builder", 0)
        for round_ in range(2):
            sp = scenes.two_object_scene(os.path.join(scenes.RES, "teapot.obj"), os.path.join(scenes.RES, "cube.obj"), 1, 0, 2, 2,
                                         sky=scenes.synthetic_skybox(32), ctx=c)
            img, st = c.trace(FW, FH)
            ref, rc = sp.orc.render(FW, FH)
            assert_frame_equals_oracle(img, sp.orc, FW, FH, ref=ref)
            assert counts(st) == tuple(int(x) for x in rc)
            res = c.intersect_device(dev(teapot_rays))
            torch.cuda.synchronize()
            assert_hits_equal_oracle(res.numpy()[0], sp.orc, teapot_rays)
            if round_ == 1:
                break
            c.upload_geometry(v, ix, ranges)
            c.set_instances(inst)
            c.set_uniforms(u)
            model = sr.StackModel(c.debug_snapshot())
            assert sr.stack2_lds() == STACK2_LDS
            peaks = [model.first(q) for q in sr.rays_of(rays[:8])]
            assert min(peaks) >= 30, peaks                    # (most of the 40 levels: far into the spill area)
            prim = centre_rays(deep_orc, FW, FH)
            assert (deep_orc.intersect(prim, use_bvh=False)["inst"] == 1).all(), "the corridor fills the view"
            fpeaks = [model.first(q) for q in sr.rays_of(prim)]
            assert min(fpeaks) >= STACK2_LDS + FRAME, fpeaks
            print("40-level tree: modelled peaks %s; primary rays of the frame: %d .. %d" % (peaks, min(fpeaks), max(fpeaks)))
            img, st = c.trace(FW, FH)
            assert_frame_equals_oracle(img, deep_orc, FW, FH, ref=deep_ref)
            assert counts(st) == tuple(int(x) for x in deep_rc)
            res = c.intersect_device(dev(rays))
            torch.cuda.synchronize()
            assert res.numpy()[0].tobytes() == deep_hits.tobytes()
    finally:
        c.close()


_DEVICE_CLOSEST = {}


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["1", "2", "3"])
def test_device_built_trees(algo, monkeypatch):
    """every device BLAS builder (RT_GPU_BVH_ALGO) under a device-built TLAS, and the deep corridor's tree after a device refit: the
    premise comes from that context's snapshot"""
    import torch
    from tests.test_ray_query import dev_inst
    w = World(builder=algo, mp=monkeypatch, device_tlas=True)
    try:
        rays, tag, whole = corridor_rays(ALL_TARGETS, 37, seed=41)
        words = flag_words(len(rays), 42)
        for step in ("built", "refitted"):
            if step == "refitted":
                ff, fi, pc = w.ranges[len(LADDER)]
                v = w.verts.copy()
                mesh_v = v[ff:ff + 6 * 4 * DEEP].reshape(-1, 6)                  # (four vertices per square)
                mesh_v[:, 0] += np.float32(0.25)                          # the deep corridor, a quarter to the side
                w.ctx.refit_blas_device(len(LADDER), torch.from_numpy(mesh_v.copy()).to("cuda:0"))
                w.ctx.set_instances_device(dev_inst(w.inst))
                w.ctx.synchronize()
                w.model = sr.StackModel(w.ctx.debug_snapshot())
                w.orc = oracle_scene(v, w.idx, w.ranges, w.inst)
            premise(w.model, sr.rays_of(rays), whole, (I_DEEP,), shallow=(), what="RT_GPU_BVH_ALGO %s, %s" % (algo, step))
            closest = w.ctx.intersect_device(dev(rays))
            first = w.ctx.intersect_device(dev(rays), any_hit=True)
            flags = w.ctx.intersect_device_flags(dev(rays), words=dev_words(words), attributes=True)
            near = np.nonzero(whole == I_DEEP)[0][:8]                     # 3 off either end of the deep corridor, no radius
            pts = np.concatenate([rays[near, 0:3] + np.float32(2.0) * rays[near, 4:7], np.full((len(near), 1), np.float32(np.inf))], axis=1)
            ppeaks = [w.model.first(sr.Point(p[0:3])) for p in pts.astype(np.float64)]
            assert len(near) == 8 and min(ppeaks) >= STACK2_LDS + SINGLE, ppeaks
            cp = w.ctx.closest_point_device(dev(pts, 4))
            torch.cuda.synchronize()
            assert_hits_equal_oracle(closest.numpy()[0], w.orc, rays)
            check_first_hits(w.orc, rays, first.numpy()[0])
            h, a = flags.numpy()
            check_against_oracle(w.orc, rays, words, 0, 0xFF, h, a, what="algo %s %s" % (algo, step))
            if step not in _DEVICE_CLOSEST:                               # (the same points and geometry under every builder)
                _DEVICE_CLOSEST[step] = cr.brute32(cr.Scene(w.verts if step == "built" else v, w.idx, w.ranges, w.inst), pts)
            assert cp.numpy()[0].tobytes() == _DEVICE_CLOSEST[step].tobytes()
    finally:
        w.ctx.close()
