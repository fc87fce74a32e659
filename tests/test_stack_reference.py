"""The CPU model of the traversal stack's peak (tests/stack_reference.py) on trees whose peak is known by construction, the corridor
ladder that tests/test_stack_spill.py walks on the GPU, and two recorded measurements of what the older scenes reach.  No GPU."""
import functools
import os

import numpy as np
import pytest

from tests import scenes, stack_reference as sr, tree_reference as tr
from vulkan_raytracing_amd import api, host
from vulkan_raytracing_amd.api import TRI_PACKET_DTYPE

STACK2_LDS = 12                      # the value these tests were written for
LADDER = (256, 512, 1024, 2048, 4096, 8192, 16384)
DEEP = 65536


def test_the_knob_is_the_one_the_tests_were_written_for():
    """a change of RT_STACK2_LDS moves the boundary: the ladder (and the margins of test_stack_spill.py) must move with it"""
    assert sr.stack2_lds() == STACK2_LDS


# ---- combs: one leaf per level --------------------------------------------------------------------------------------------------------

def comb(levels, left):
    """a snapshot of one mesh of levels + 1 unit squares, square i in the plane z = -i, under a comb of `levels` interior nodes: the
    left comb (((0, 1), 2), 3) ... keeps its subtree in child 0 and a leaf in child 1, the right comb (0, (1, (2, 3))) ... the other
    way round.  Square 0 is the deepest leaf of the left comb and the shallowest of the right one."""
    n = levels + 1
    v, ix = scenes.corridor(n, spacing=1.0)
    v[:, :2] /= scenes.CORRIDOR_SIDE
    topo = 0
    if left:
        for i in range(1, n):
            topo = (topo, i)
    else:
        topo = n - 1
        for i in range(n - 2, -1, -1):
            topo = (i, topo)
    pos = v[:, :3].astype(np.float64)
    q_lo, q_s = tr.quant_params(pos.min(axis=0), pos.max(axis=0))
    box = lambda i: (pos[4 * i:4 * i + 4].min(axis=0), pos[4 * i:4 * i + 4].max(axis=0))
    nodes = tr.build_tree(topo, box, lambda i: ((2 * i) << 3) | 1, q_lo, q_s)          # leaf i: packets 2i and 2i + 1
    assert len(nodes) == levels and sr.tree_levels(nodes) == levels
    snap, _ = tr.link_meshes([(v, ix, nodes, np.zeros(2 * n, TRI_PACKET_DTYPE), q_lo, q_s, levels)])
    return snap


L = 17
DOWN = sr.Ray((0.1, 0.2, 5.0), (0.0, 0.0, -1.0))
UP = sr.Ray((0.1, 0.2, -L - 5.0), (0.0, 0.0, 1.0))
ALL = sr.Box((-1, -1, -L - 1), (1, 1, 1))
FRONT, BEHIND = sr.Point((0.1, 0.2, 5.0)), sr.Point((0.1, 0.2, -L - 5.0))


def test_combs_peak_by_the_rule_and_the_order():
    """A one-instance TLAS adds the sentinel and the marker: 2.  A walk that always descends into the comb's subtree keeps one leaf
    per level: L + 2.  A walk that always takes the leaf first keeps the subtree, pops it and goes on: 1 + 2."""
    left, right = sr.StackModel(comb(L, True)), sr.StackModel(comb(L, False))
    # child 0 first: the left comb's subtrees are child 0
    assert left.peak(ALL, full=True) == (L + 2, L + 2) and right.peak(ALL, full=True) == (3, 3)
    assert left.peak(ALL, full=True, blas_only=0) == (L, L) and right.peak(ALL, full=True, blas_only=0) == (1, 1)
    # nearer first: by the ray's direction.  The left comb's subtrees hold square 0 (z = 0), the right comb's the last square (z = -L)
    for m, near, far in ((left, DOWN, UP), (left, FRONT, BEHIND), (right, UP, DOWN), (right, BEHIND, FRONT)):
        assert m.peak(near, full=True) == (L + 2, L + 2), "coming from the subtree's end, the subtree is nearer at every level"
        assert m.peak(far, full=True) == (3, 3), "coming from the other end, the leaf is nearer at every level"
    # a search radius that ends before the row does: the walk never enters what lies beyond it
    assert left.peak(sr.Point((0.1, 0.2, 5.0), radius=5.5), full=True) == (2, 2)        # only square 0 is within 5.5: the sentinel and the marker
    # a ray that misses everything holds the sentinel alone
    assert left.peak(sr.Ray((5, 5, 5), (0, 0, -1)), full=True) == (1, 1)
    # a swept sphere wide enough reaches the row from beside it
    assert left.first(sr.Ray((1.5, 0.0, 5.0), (0.0, 0.0, -1.0), r=1.0)) == L + 2


# ---- the corridor ladder ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def corridor_model(n):
    v, ix = scenes.corridor(n)
    rc, info = api.check_builders(v, ix)
    assert rc == 0 and info["violations"] == 0, info
    snap = sr.host_snapshot([(v, ix)])
    return sr.StackModel(snap), int(snap["meshes"]["levels"][0]), info


def corridor_queries(n, seed, count=6, x0=0.0):
    """rays down and up the row inside the footprint, a box that covers it, a point in front of it, a sphere swept along it"""
    rng = np.random.default_rng(seed)
    length = scenes.corridor_length(n)
    qs = []
    for i in range(count):
        a = np.array([x0 + rng.uniform(-7, 7), rng.uniform(-7, 7), 5.0])
        b = np.array([x0 + rng.uniform(-7, 7), rng.uniform(-7, 7), -length - 5.0])
        if i % 2:
            a, b = b, a
        qs.append(sr.Ray(a, (b - a) / np.linalg.norm(b - a), 0.001, 10000.0, r=0.25 * (i % 3 == 2)))
    qs.append(sr.Box((x0 - 9, -9, -length - 1), (x0 + 9, 9, 1)))
    qs.append(sr.Point((x0 + 1.0, 2.0, 3.0)))
    return qs


def test_the_ladder_takes_every_value_across_the_boundary():
    """The host builder halves a corridor at every level; every query along it holds one entry per level, the marker and the
    sentinel.  Ladder: full peaks STACK2_LDS - 3 .. STACK2_LDS + 3, one mesh each; the deep mesh: STACK2_LDS + 5."""
    peaks = {}
    for n in LADDER + (DEEP,):
        model, levels, info = corridor_model(n)
        assert info["depth"] == levels == int(np.log2(n)) - 1, (n, info)
        for q in corridor_queries(n, seed=n):
            assert model.peak(q, blas_only=0)[0] == levels, (n, q.rule)
            assert model.first(q) == levels + 2, (n, q.rule)
        peaks[n] = levels + 2
    assert [peaks[n] for n in LADDER] == list(range(STACK2_LDS - 3, STACK2_LDS + 4))
    assert peaks[DEEP] >= STACK2_LDS + 5
    # the all-hits walk of the whole row is no deeper than its first descent
    model, levels, _ = corridor_model(1024)
    for q in corridor_queries(1024, seed=3, count=2):
        assert model.peak(q, full=True) == (levels + 2, levels + 2)


# ---- recorded measurements: what the older scenes reach ------------------------------------------------------------------------------

def chain_mesh(n=120, s=0.5):
    """n copies of one large triangle (x 80 .. 140, y -20 .. 40) stacked below the plane z = 0 at z = -4 s^k.  The frame half of
    test_launch_tunables.test_spill_areas_grow_with_the_grid used this mesh, on the argument that a ray down through the footprint
    enters every box of its 28-level tree."""
    v = np.zeros((n, 3, 6), np.float32)
    v[:, :, 0] = (80.0, 140.0, 80.0)
    v[:, :, 1] = (-20.0, -20.0, 40.0)
    v[:, :, 2] = (-4.0 * s ** np.arange(n))[:, None]
    v[:, :, 5] = 1.0
    return v.reshape(-1, 6), np.arange(3 * n, dtype=np.uint32)


def test_recorded_the_chain_mesh_does_not_spill():
    """Recorded experiment.  The tree has 28 levels, but the planes are spaced geometrically in z only: below about 16 octaves their
    16-bit z planes coincide, the tied children are taken in order, and the walk never holds more than a few siblings.  300 rays
    from that test's camera position (100, 0, 6) through its view: every peak is far below STACK2_LDS.  Measured: 5 pending BLAS
    entries at most (7 with the sentinel and the marker)."""
    v, ix = chain_mesh()
    rc, info = api.check_builders(v, ix)
    assert rc == 0 and info["depth"] >= 24
    model = sr.StackModel(sr.host_snapshot([(v, ix)]))
    rng = np.random.default_rng(9)
    peaks = []
    for _ in range(300):
        d = np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.5, 0.5), -1.0])
        peaks.append(model.peak(sr.Ray((100.0, 0.0, 6.0), d / np.linalg.norm(d), 0.001, 10000.0), full=True)[1])
    assert max(peaks) <= 7 < STACK2_LDS, max(peaks)


def test_recorded_the_teapot_never_comes_near_the_boundary():
    """Recorded experiment.  The teapot's BLAS has 13 levels; 1500 random rays walked as all-hits (nothing pruned: an upper bound of
    every ray walk) hold at most 9 pending BLAS entries.  With the sentinel and the marker that is 11: a scene of a few
    instances of it stays inside the LDS part."""
    g = host.SceneGeometry([os.path.join(scenes.RES, "teapot.obj")])
    v, ix = g.verts.reshape(-1, 6), g.idx
    model = sr.StackModel(sr.host_snapshot([(v, ix)]))
    assert int(model.snap["meshes"]["levels"][0]) == 13
    rays = scenes.random_rays(1500, seed=17, origin_radius=12.0, target_radius=2.0)
    peaks = np.array([model.peak(r, full=True, blas_only=0)[1] for r in sr.rays_of(rays)])
    assert peaks.max() <= 9 and peaks.max() + 2 < STACK2_LDS, peaks.max()
    assert (peaks >= 8).mean() < 0.01
