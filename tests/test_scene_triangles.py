"""rt_scene_triangles_device, rt_overlap_scene_triangles* and rt_closest_scene_triangle*: the two triangle queries asked about triangles
of the scene itself, named by (inst, prim, against, r_max) references.

tests/scene_triangle_reference.py holds the reference: the records from closest_reference.Scene's canonical transforms, then
triangle_overlap_reference's predicate and triangle_distance_reference's feature sequence over them with the instance rule (against ==
-1: not the source's instance; against >= 0: that instance only) in front of the rows and of the key's minimum.  It is the same
canonical arithmetic as the plain calls', so everything is held byte for byte.  The CPU part asserts the premises of the GPU tests on the
reference alone (the scenes exercise the rule), the exports, the packing and the kernels' register budget."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import closest_reference as cr
from tests import scene_triangle_reference as stf
from tests import triangle_distance_reference as tdr
from tests import triangle_overlap_reference as trf
from tests.test_closest_point import small_scene
from tests.test_ray_query import PATHS, dev_inst, slow_queue
from tests.test_ray_query_oracle import oracle_scene, use_builder
from vulkan_raytracing_amd import RtContext, api
from vulkan_raytracing_amd.api import HIT_DTYPE, RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
F = np.float32
ME = 5   # the instance of the mask cross-check


# ---- scenes and their references, computed once -----------------------------------------------------------------------------

def scene_parts(name):
    """`far`: small_scene(seed=157) as it is (32 instances of an octahedron and a 12-triangle soup, 320 triangles, eight masks including 0;
    sheared, mirrored and scaled); `close`: its translations x 0.3, the bodies interpenetrate; `masks`: close with mask 0x01 on instance
    ME and 0x02 on the rest; `moved`: close with every translation shifted a little (the TLAS update)"""
    verts, idx, ranges, inst = small_scene(seed=157)
    inst = inst.copy()
    if name != "far":
        inst["transform"][:, [3, 7, 11]] *= F(0.3)
    if name == "masks":
        for i in range(len(inst)):
            inst[i]["custom_index_and_mask"] = (int(inst[i]["custom_index_and_mask"]) & 0xFFFFFF) | ((0x01 if i == ME else 0x02) << 24)
    if name == "moved":
        inst["transform"][:, [3, 7, 11]] += np.random.default_rng(158).uniform(-0.2, 0.2, (len(inst), 3)).astype(F)
    return verts, idx, ranges, inst


class Case:
    def __init__(self, parts):
        self.parts = parts
        self.sc = cr.Scene(*parts)
        self.src = stf.Source(self.sc, *parts)
        self.n_inst = len(parts[3])
        self._memo = {}

    def overlaps(self, refs, cull=0xFF, max_ids=16, rule=True):
        key = ("o", refs.tobytes(), cull, max_ids, rule)
        if key not in self._memo:
            self._memo[key] = stf.overlaps(self.src, refs, cull, max_ids, rule)
        return self._memo[key]

    def nearest(self, refs, cull=0xFF, rule=True):
        key = ("n", refs.tobytes(), cull, rule)
        if key not in self._memo:
            self._memo[key] = stf.nearest(self.src, refs, cull, rule)
        return self._memo[key]


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = Case(scene_parts(name))
    return _CASES[name]


def pair_refs(c, n_first=8):
    """every triangle of a against b for every ordered pair (a, b) of the first n_first instances, a == b included"""
    sel = np.nonzero(c.sc.inst < n_first)[0]
    return np.concatenate([stf.refs(c.sc.inst[sel], c.sc.prim[sel], b) for b in range(n_first)])


def half_radii(c, refs):
    """the references with finite radii about the median distance of their answers, so that about half of them miss"""
    t = c.nearest(refs)[0]["t"]
    r = refs.copy()
    r[:, 3] = np.full(len(r), np.median(t), F).view(np.int32)
    return r


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------

def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def load(ctx, parts, device=False, update=False):
    import torch
    verts, idx, ranges, inst = parts
    if not update:
        ctx.upload_geometry(verts, idx, ranges)
    if device:
        torch.cuda.synchronize()
        ctx.set_instances_device(dev_inst(inst), update=update)
    else:
        ctx.set_instances(inst, update=update)


def gpu_overlap(ctx, refs, cull=0xFF, **kw):
    import torch
    res = ctx.overlap_scene_triangles_device(dev(refs), cull_mask=cull, **kw)
    torch.cuda.synchronize()
    return res.numpy()


def gpu_nearest(ctx, refs, cull=0xFF, attributes=True, params=True):
    import torch
    res = ctx.closest_scene_triangle_device(dev(refs), cull_mask=cull, attributes=attributes, params=params)
    torch.cuda.synchronize()
    h, a = res.numpy()
    return h, a, (res.quv.cpu().numpy() if res.quv is not None else None)


def same(got, want, what, max_ids=16):
    counts, ids = got
    rc, ri = want
    if counts is not None:
        assert counts.tobytes() == rc.tobytes(), (what, np.nonzero(counts != rc)[0][:5], counts[counts != rc][:5], rc[counts != rc][:5])
    if ids is not None:
        ri = np.ascontiguousarray(ri[:, :max_ids])
        assert ids.tobytes() == ri.tobytes(), (what, np.nonzero((ids != ri).any(axis=(1, 2)))[0][:5])


def overlap_modes(ctx, c, refs, cull, what):
    """counts and ids with max_ids 16, max_ids 3 without counts (the walk prunes), max_ids 0, and occupancy"""
    want = c.overlaps(refs, cull)
    same(gpu_overlap(ctx, refs, cull, max_ids=16), want, what + ", 16 ids")
    counts, ids = gpu_overlap(ctx, refs, cull, max_ids=3, counts=False)
    assert counts is None
    same((None, ids), want, what + ", 3 ids without counts", max_ids=3)
    counts, ids = gpu_overlap(ctx, refs, cull, max_ids=0)
    assert ids is None
    same((counts, None), want, what + ", counts only")
    occ, _ = gpu_overlap(ctx, refs, cull, max_ids=0, any=True)
    assert np.array_equal(occ, (want[0] > 0).astype(np.uint32)), what + ", any"
    return want


def nearest_check(ctx, c, refs, cull=0xFF, what="", orc=None, attributes=True):
    """hits and (qu, qv) against the reference byte for byte; with orc the attributes against the oracle's of the returned records and the
    restated side words at the source triangle's point"""
    h, a, quv = gpu_nearest(ctx, refs, cull, attributes=attributes and orc is not None)
    ref, q_ref = c.nearest(refs, cull)
    if h.tobytes() != ref.tobytes():
        bad = np.nonzero((h.view(np.uint8).reshape(len(h), -1) != ref.view(np.uint8).reshape(len(h), -1)).any(axis=1))[0]
        raise AssertionError("%s: %d records differ, first %d: reference %s gpu %s expected %s" % (what, len(bad), bad[0], refs[bad[0]], h[bad[0]], ref[bad[0]]))
    assert quv.tobytes() == q_ref.tobytes(), what
    if a is not None:
        tris = stf.expand(c.src, refs)[0]
        kinds, _ = tdr.side_words(c.sc, tris, ref, q_ref)
        assert np.array_equal(a[:, 7].view(np.uint32), kinds), what
        o = orc.hit_attributes(np.ascontiguousarray(h))
        f = a.view(F)
        assert np.array_equal(f[:, 0:3].view(np.uint32), o[:, 0:3].view(np.uint32)) and np.array_equal(f[:, 4:7].view(np.uint32), o[:, 3:6].view(np.uint32)), what
        assert np.array_equal(a[:, 3], o[:, 6].astype(np.int32)), what
        miss = h["inst"] < 0
        assert (a[miss, 0:3] == 0).all() and (a[miss, 4:7] == 0).all() and (a[miss, 7] == 0).all() and (a[miss, 3] == -1).all(), what
    return ref, q_ref


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

NEW = ("rt_scene_triangles_device", "rt_overlap_scene_triangles_device", "rt_overlap_scene_triangles", "rt_closest_scene_triangle_device",
       "rt_closest_scene_triangle")


def test_exports_abi_and_null_context():
    for name in NEW:
        assert name in api.EXPORTS, name
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^#define RT_REF_AGAINST_OTHERS \(-1\)$", hdr, re.M)
    assert re.search(r"typedef struct rt_tri_ref \{\s+int32_t inst;[^}]*int32_t prim;[^}]*int32_t against;[^}]*float\s+r_max;[^}]*\} rt_tri_ref;", hdr)
    assert re.search(r"^int rt_scene_triangles_device\(rt_ctx\* ctx, size_t n, const void\* d_refs4, void\* d_tris12, void\* hip_stream\);", hdr, re.M)
    assert re.search(r"^int rt_overlap_scene_triangles_device\(rt_ctx\* ctx, size_t n, const void\* d_refs4, uint32_t cull_mask, uint32_t flags,\s+uint32_t max_ids, "
                     r"void\* d_ids, void\* d_counts, void\* hip_stream\);", hdr, re.M)
    assert re.search(r"^int rt_overlap_scene_triangles\(rt_ctx\* ctx, size_t n, const rt_tri_ref\* refs_host, uint32_t cull_mask, uint32_t flags,\s+uint32_t max_ids, "
                     r"int32_t\* ids_host, uint32_t\* counts_host, int counting, rt_stats\* stats\);", hdr, re.M)
    assert re.search(r"^int rt_closest_scene_triangle_device\(rt_ctx\* ctx, size_t n, const void\* d_refs4, uint32_t cull_mask,\s+void\* d_hits, void\* d_attr, "
                     r"void\* d_params, void\* hip_stream\);", hdr, re.M)
    assert re.search(r"^int rt_closest_scene_triangle\(rt_ctx\* ctx, size_t n, const rt_tri_ref\* refs_host, uint32_t cull_mask,\s+rt_hit\* out_host, "
                     r"float\* params_host, int counting, rt_stats\* stats\);", hdr, re.M)
    L = api.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert L.rt_abi_version() == 7
    assert L.rt_scene_triangles_device(None, 0, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_overlap_scene_triangles_device(None, 64, None, 0xFF, 0, 4, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_overlap_scene_triangles(None, 0, None, 0xFF, 0, 0, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_closest_scene_triangle_device(None, 0, None, 0xFF, None, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_closest_scene_triangle(None, 0, None, 0xFF, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
    for name in ("scene_triangles_device", "overlap_scene_triangles_device", "overlap_scene_triangles", "closest_scene_triangle_device", "closest_scene_triangle"):
        assert hasattr(RtContext, name), name
    assert api.TRI_REF_DTYPE.itemsize == 16 and api.TRI_REF_DTYPE.names == ("inst", "prim", "against", "r_max") and api.REF_AGAINST_OTHERS == -1


def test_triangle_refs_pack_as_specified():
    r = api.triangle_refs([3, 4, 2 ** 31 - 1], [0, 7, -1])
    assert r.dtype == np.int32 and r.shape == (3, 4) and r.flags["C_CONTIGUOUS"]
    assert r[:, 0].tolist() == [3, 4, 2 ** 31 - 1] and r[:, 1].tolist() == [0, 7, -1] and (r[:, 2] == -1).all()
    assert (r[:, 3].view(np.uint32) == 0x7F800000).all()   # r_max = +inf
    r = api.triangle_refs(5, np.arange(4), against=[1, 2, 3, -1], r_max=np.array([0.5, np.nan, -0.0, 3e38], F))
    v = r.view(api.TRI_REF_DTYPE).reshape(-1)
    assert (v["inst"] == 5).all() and v["prim"].tolist() == [0, 1, 2, 3] and v["against"].tolist() == [1, 2, 3, -1]
    assert v["r_max"].view(np.uint32).tolist() == np.array([0.5, np.nan, -0.0, 3e38], F).view(np.uint32).tolist()
    assert np.array_equal(r, stf.refs(5, np.arange(4), [1, 2, 3, -1], np.array([0.5, np.nan, -0.0, 3e38], F)))
    assert api.triangle_refs(np.zeros(0, np.int64), np.zeros(0, np.int64)).shape == (0, 4)
    import torch
    t = api.triangle_refs(torch.tensor([3, 4]), torch.tensor([0, 7]), against=2, r_max=1.5)
    assert t.dtype == torch.int32 and tuple(t.shape) == (2, 4) and t.is_contiguous()
    assert np.array_equal(t.numpy(), api.triangle_refs([3, 4], [0, 7], 2, 1.5))


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_scene_triangle_kernels_keep_the_record_level_budget(target):
    """exactly two k_refs_collide* and two k_refs_nearest* kernels in both libraries, each within the record-level walks' budget (>= 4
    waves per SIMD, scratch <= 32 bytes, no spills, the 12 KB stack in LDS); k_refs_expand without scratch or spills"""
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    for stem in ("k_refs_collide", "k_refs_nearest"):
        walk = [(n, r) for n, r in kernels.items() if stem in n]
        assert len(walk) == 2 and sum(stem + "_count" in n for n, _ in walk) == 1, "\n".join(kernels)
        for name, r in walk:
            assert int(r["Occupancy"]) >= 4 and int(r["ScratchSize"]) <= 32 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
            assert int(r["LDS Size"]) == 12288, (name, r)
    ex = [(n, r) for n, r in kernels.items() if "k_refs_expand" in n]
    assert len(ex) == 1
    assert int(ex[0][1]["ScratchSize"]) == 0 and int(ex[0][1]["VGPRs Spill"]) == 0 and int(ex[0][1]["SGPRs Spill"]) == 0, ex


def test_the_scenes_exercise_the_rule():
    """the premises of the GPU tests, on the reference alone"""
    c = case("close")
    assert c.n_inst == 32 and c.sc.n_tris == 320 and len(np.unique(c.sc.mask)) == 8 and (c.sc.mask == 0).any()
    every = stf.every_triangle(c.sc)
    counts, ids = c.overlaps(every)
    plain, _ = c.overlaps(every, rule=False)
    print("close scene: %d of 320 records overlap another body, %d have more than 16 candidates, %d counts change by the exclusion" %
          ((counts > 0).sum(), (counts > 16).sum(), (counts != plain).sum()))
    assert (counts > 0).sum() >= 250 and (counts > 16).sum() >= 30 and (counts != plain).sum() >= 200
    assert (ids[..., 0] != every[:, 0:1]).all()      # (-1 past the last entry differs too)
    # against == inst: every valid record of an admitted instance lists itself; the records of mask-0 instances come back empty
    own = stf.every_triangle(c.sc, against=c.sc.inst)
    oc, oi = c.overlaps(own, max_ids=16)
    admitted = c.sc.admitted(0xFF)
    listed = ((oi[..., 0] == own[:, 0:1]) & (oi[..., 1] == own[:, 1:2])).any(axis=1)
    assert admitted.sum() == 280 and (oc[~admitted] == 0).all() and (oc[admitted] >= 1).all()
    assert listed[admitted & (oc <= 16)].all() and (oc <= 16)[admitted].mean() > 0.9
    assert (oi[..., 0][oi[..., 0] >= 0] == np.broadcast_to(own[:, 0:1], oi[..., 0].shape)[oi[..., 0] >= 0]).all()
    # the distance query on the unscaled scene
    f = case("far")
    every = stf.every_triangle(f.sc)
    h, quv = f.nearest(every)
    hp, _ = f.nearest(every, rule=False)
    print("far scene: t of the nearest other body %.3g .. %.3g, median %.3g; the plain call answers the source's own instance for %d records" %
          (h["t"].min(), h["t"].max(), np.median(h["t"]), (hp["inst"] == every[:, 0]).sum()))
    assert (h["inst"] >= 0).all() and (h["inst"] != every[:, 0]).all() and (h["t"] > 1e-3).all()
    assert (hp["inst"] == every[:, 0]).sum() == 280
    half = half_radii(f, every)
    hh, _ = f.nearest(half)
    assert 0.3 < (hh["inst"] < 0).mean() < 0.7
    assert np.array_equal(hh["t"][hh["inst"] < 0].view(np.uint32), half[hh["inst"] < 0, 3].view(np.uint32))
    # pierced sources on the close scene report the crossing residue, as the reference has it
    hc, _ = c.nearest(stf.every_triangle(c.sc))
    pierced = counts > 0
    assert (hc["inst"][pierced] >= 0).all() and np.median(hc["t"][pierced]) < 1e-3 < np.median(h["t"])


def test_invalid_references_on_the_reference():
    c = case("close")
    n = c.n_inst
    r = stf.refs([-1, n, 2 ** 31 - 1, 0, 0, 0, 0, 0, 1], [0, 0, 0, -1, int(c.src.count[0]), 2 ** 31 - 1, 0, 0, 0], [-1, -1, -1, -1, -1, -1, -2, n, 0], 2.5)
    q, ok, _ = stf.expand(c.src, r)
    assert not ok[:8].any() and ok[8]
    assert (q.view(np.uint32)[:8][:, trf.COLS] == 0x7FC00000).all() and np.array_equal(q.view(np.int32)[:, [7, 11]], r[:, [0, 2]])
    assert (q[:, 3] == 2.5).all()
    counts, ids = c.overlaps(r)
    assert (counts[:8] == 0).all() and (ids[:8] == -1).all()
    h, quv = c.nearest(r)
    assert (h["inst"][:8] == -1).all() and (h["t"][:8] == 2.5).all() and (quv[:8] == 0).all()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


@pytest.mark.gpu
def test_expansion(ctx):
    """scene_triangles_device over every (inst, prim) equals the reference's records in all twelve words; invalid references (inst, prim
    and against out of range, an instance with a NaN transform, bad vertices) give nine NaNs with words 3 / 7 / 11 kept, and RT_OK"""
    import torch
    from tests import bad_vertex_cases as bvc
    verts, idx, ranges, inst = scene_parts("far")
    c = case("far")
    load(ctx, c.parts)
    every = stf.every_triangle(c.sc, against=np.arange(320) % 33 - 1, r_max=np.linspace(0, 9, 320).astype(F))
    got = ctx.scene_triangles_device(dev(every))
    torch.cuda.synchronize()
    want, ok, _ = stf.expand(c.src, every)
    assert ok.all() and got.cpu().numpy().tobytes() == want.tobytes()
    # the same scene with a NaN transform on instance 7 and two bad vertices in the soup
    verts = np.array(verts, F, copy=True)
    inst = inst.copy()
    inst[7]["transform"][5] = np.nan
    ff, fi, pc = ranges[1]
    pos = verts[ff:].reshape(-1, 6)[:, :3]            # (a view: the makers write into the buffer)
    tri = np.asarray(idx[fi:fi + 3 * pc], np.int64).reshape(-1, 3)
    bvc.BAD["nan_y"](pos, np.array([tri[3, 0]]), tri)
    bvc.BAD["1e37_y"](pos, np.array([tri[7, 1]]), tri)
    with np.errstate(all="ignore"):
        b = Case((verts, idx, ranges, inst))
    load(ctx, b.parts)
    n = b.n_inst
    bad = stf.refs([-1, n, 2 ** 31 - 1, 0, 0, 0, 3, 3], [0, 0, 0, -1, int(b.src.count[0]), 2 ** 31 - 1, 0, 0], [-1, -1, -1, -1, -1, -1, -2, n],
                   np.array([1.0, np.nan, -1.0, np.inf, 0.0, 2.0, 3.0, 4.0], F))
    refs = np.concatenate([bad, stf.every_triangle(b.sc, r_max=1.5)])
    got = ctx.scene_triangles_device(dev(refs))
    torch.cuda.synchronize()
    want, ok, _ = stf.expand(b.src, refs)
    on7 = refs[:, 0] == 7
    soup = np.array([int(inst[i]["mesh"]) == 1 for i in range(n)])
    assert not ok[:8].any() and not ok[on7].any() and on7.sum() > 0
    assert b.src.bad.sum() >= 2 * soup.sum() and (~ok[8:][b.src.bad]).all() and ok.sum() > 250
    g = got.cpu().numpy()
    assert g.tobytes() == want.tobytes(), np.nonzero((g.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0][:5]
    assert (g.view(np.uint32)[~ok][:, trf.COLS] == 0x7FC00000).all()
    # invalid references are answered, not refused: count 0 and an empty row, the miss record with t = r_max as given
    counts, ids = gpu_overlap(ctx, bad, max_ids=4)
    assert (counts == 0).all() and (ids == -1).all()
    h, a, quv = gpu_nearest(ctx, bad)
    assert (h["inst"] == -1).all() and (h["prim"] == -1).all() and np.array_equal(h["t"].view(np.uint32), bad[:, 3].view(np.uint32))
    assert (quv == 0).all() and (a[:, [0, 1, 2, 4, 5, 6, 7]] == 0).all() and (a[:, 3] == -1).all()
    # the output feeds the plain calls directly
    t = ctx.scene_triangles_device(dev(stf.every_triangle(b.sc)))
    plain = ctx.overlap_triangles_device(t, max_ids=16)
    torch.cuda.synchronize()
    assert (plain.count.cpu().numpy()[~stf.expand(b.src, stf.every_triangle(b.sc))[1]] == 0).all()


@pytest.mark.gpu
def test_overlaps_against_the_others(ctx):
    c = case("close")
    load(ctx, c.parts)
    every = stf.every_triangle(c.sc)
    overlap_modes(ctx, c, every, 0xFF, "close scene")
    for cull in (0x5A, 0x01, 0x00):
        same(gpu_overlap(ctx, every, cull, max_ids=16), c.overlaps(every, cull), "close scene, cull %#x" % cull)
    # the GPU against itself: a source that the mask leaves out anyway, and one that is admitted and excluded by rule
    import torch
    m = case("masks")
    load(ctx, m.parts)
    mine = every[every[:, 0] == ME]
    out = gpu_overlap(ctx, mine, 0x02, max_ids=16)
    by_rule = gpu_overlap(ctx, mine, 0x03, max_ids=16)
    assert out[0].tobytes() == by_rule[0].tobytes() and out[1].tobytes() == by_rule[1].tobytes()
    plain = ctx.overlap_triangles_device(ctx.scene_triangles_device(dev(mine)), max_ids=16, cull_mask=0x02)
    torch.cuda.synchronize()
    plain = plain.numpy()
    assert out[0].tobytes() == plain[0].tobytes() and out[1].tobytes() == plain[1].tobytes()
    same(out, m.overlaps(mine, 0x02), "instance %d under 0x02" % ME)
    assert (out[0] > 0).sum() >= 3


@pytest.mark.gpu
def test_pairs_of_instances(ctx):
    c = case("close")
    load(ctx, c.parts)
    pairs = pair_refs(c)
    want = overlap_modes(ctx, c, pairs, 0xFF, "pairs")
    assert (want[0] > 0).sum() > 50
    inst_ids = want[1][..., 0]
    assert (inst_ids[inst_ids >= 0] == np.broadcast_to(pairs[:, 2:3], inst_ids.shape)[inst_ids >= 0]).all()
    own = stf.every_triangle(c.sc, against=c.sc.inst)
    counts, ids = gpu_overlap(ctx, own, max_ids=16)
    same((counts, ids), c.overlaps(own), "against == inst")
    admitted = c.sc.admitted(0xFF)
    assert (counts[~admitted] == 0).all() and (ids[~admitted] == -1).all() and (counts[admitted] >= 1).all()
    # an `against` whose instance the cull mask rejects gives count 0
    for cull in (0x01, 0x10):
        counts, ids = gpu_overlap(ctx, pairs, cull, max_ids=16)
        same((counts, ids), c.overlaps(pairs, cull), "pairs, cull %#x" % cull)
        rejected = (c.sc.mask[pairs[:, 2]] & cull) == 0
        assert rejected.any() and (counts[rejected] == 0).all() and (counts[~rejected] > 0).any()


@pytest.mark.gpu
def test_distances(ctx):
    f = case("far")
    load(ctx, f.parts)
    orc = oracle_scene(*f.parts)
    every = stf.every_triangle(f.sc)
    ref, _ = nearest_check(ctx, f, every, what="far scene", orc=orc)
    assert (ref["inst"] >= 0).all() and (ref["t"] > 1e-3).all()
    half = half_radii(f, every)
    ref, _ = nearest_check(ctx, f, half, what="far scene, finite radii", orc=orc)
    assert 0.3 < (ref["inst"] < 0).mean() < 0.7
    pairs = pair_refs(f)
    ref, _ = nearest_check(ctx, f, pairs, what="far scene, pairs", orc=orc)
    assert (ref["inst"][ref["inst"] >= 0] == pairs[ref["inst"] >= 0, 2]).all() and (ref["inst"] >= 0).mean() > 0.8
    nearest_check(ctx, f, pairs, 0x5A, what="far scene, pairs, cull", orc=orc)
    nearest_check(ctx, f, every, 0x5A, what="far scene, cull", orc=orc)
    h, a, quv = gpu_nearest(ctx, every, attributes=True, params=False)      # (the side words come from the workspace's parameters)
    assert quv is None and h.tobytes() == f.nearest(every)[0].tobytes()
    assert np.array_equal(a[:, 7].view(np.uint32), tdr.side_words(f.sc, stf.expand(f.src, every)[0], *f.nearest(every))[0])
    c = case("close")
    load(ctx, c.parts)
    nearest_check(ctx, c, stf.every_triangle(c.sc), what="close scene (pierced sources)", orc=oracle_scene(*c.parts))


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "unset", "1", "2"])
def test_tree_independence(builder, monkeypatch):
    c, f = case("close"), case("far")
    ctx = RtContext(0)
    try:
        if builder == "unset":
            monkeypatch.delenv("RT_GPU_BVH_ALGO", raising=False)
            ctx.set_param("blas_builder", 1)
        else:
            use_builder(ctx, builder, monkeypatch)
        load(ctx, c.parts)
        every = stf.every_triangle(c.sc)
        overlap_modes(ctx, c, every, 0xFF, "builder " + builder)
        load(ctx, f.parts)
        nearest_check(ctx, f, stf.every_triangle(f.sc), what="builder " + builder)
        nearest_check(ctx, f, half_radii(f, stf.every_triangle(f.sc)), what="radii, builder " + builder)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["rt_set_instances", "rt_set_instances_device"])
def test_both_record_producers(device):
    """the triangle count reaches the records whichever call made them, and a TLAS update keeps it"""
    c, m = case("close"), case("moved")
    ctx = RtContext(0)
    try:
        load(ctx, c.parts, device)
        every = stf.every_triangle(c.sc)
        pairs = pair_refs(c)
        overlap_modes(ctx, c, every, 0xFF, "built")
        overlap_modes(ctx, c, pairs, 0xFF, "built, pairs")
        assert (ctx.debug_snapshot()["instances"]["prim_count"] == c.src.count).all()
        load(ctx, m.parts, device, update=True)
        overlap_modes(ctx, m, every, 0xFF, "updated")
        overlap_modes(ctx, m, pair_refs(m), 0xFF, "updated, pairs")
        nearest_check(ctx, m, every[::3], what="updated")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_refit():
    """after rt_refit_blas_device with perturbed vertices and a TLAS update the by-reference answers are those of a fresh upload and build
    over the new vertices: the reference names the triangle, it does not copy it"""
    import torch
    from tests.test_blas_refit import deform, with_mesh
    verts, idx, ranges, inst = scene_parts("close")
    geom = types.SimpleNamespace(verts=verts, idx=idx, ranges=ranges)
    a, b = RtContext(0), RtContext(0)
    try:
        load(a, (verts, idx, ranges, inst), device=True)
        v2 = verts
        for mesh in (0, 1):
            t = deform(geom, mesh, amp=0.1)
            torch.cuda.synchronize()
            a.refit_blas_device(mesh, t)
            v2 = with_mesh(geom, v2, mesh, t)
        torch.cuda.synchronize()
        a.set_instances_device(dev_inst(inst), update=True)
        new = Case((v2, idx, ranges, inst))
        load(b, new.parts)
        every = stf.every_triangle(new.sc)
        refs = np.concatenate([every, pair_refs(new, 4)])
        ta, tb = a.scene_triangles_device(dev(refs)), b.scene_triangles_device(dev(refs))
        torch.cuda.synchronize()
        assert ta.cpu().numpy().tobytes() == tb.cpu().numpy().tobytes() == stf.expand(new.src, refs)[0].tobytes()
        assert ta.cpu().numpy().tobytes() != stf.expand(case("close").src, refs)[0].tobytes()
        ga, gb = gpu_overlap(a, refs, max_ids=16), gpu_overlap(b, refs, max_ids=16)
        assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes()
        same(ga, new.overlaps(refs), "refit")
        na, nb = gpu_nearest(a, refs), gpu_nearest(b, refs)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(na, nb))
        nearest_check(a, new, refs, what="refit")
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_the_spill_half_of_the_stack():
    """tests/test_stack_spill's small world with one more body: a copy of the shortest corridor laid lengthwise through the deepest one
    (S_TOP), so that each of its triangles spans that corridor and cuts its squares.  Premise, on the context's own snapshot: the walk of
    S_TOP's BLAS alone with a record's bounds (the overlap walk's box) or its triangle (the distance walk) has its pending entries, and
    beneath them the kernel keeps the sentinel and the instance marker in either form (against the others: further TLAS entries too);
    together they reach STACK2_LDS + 2 entries before the first triangle is tested, as in tests/test_stack_spill.py"""
    from tests import scenes
    from tests import stack_reference as sr
    from tests import test_stack_spill as tss
    from tests.test_closest_triangle import TriangleQuery
    from vulkan_raytracing_amd import host
    w = tss.World(placed=tss.PLACED_SMALL)
    try:
        n_top = tss.squares_of(tss.S_TOP, tss.PLACED_SMALL)
        length = scenes.corridor_length(n_top, tss.SPACING[n_top])
        h = scenes.CORRIDOR_SIDE / 2
        depth0 = scenes.corridor_length(tss.MESHES[0], tss.SPACING[tss.MESHES[0]])
        x_top = tss.o2w(tss.S_TOP, tss.PLACED_SMALL)[0, 3]
        # object x -> world z (the length of the corridor and 5 beyond either end), y -> 0.4 y, z -> world x (the 256 squares within 2 units)
        M = np.array([[0.0, 0.0, 2.0 / depth0, x_top + 1.0], [0.0, 0.4, 0.0, 0.0], [(length + 10.0) / (2 * h), 0.0, 0.0, -length / 2]])
        extra = host.make_instance(M.astype(F).reshape(12), 99, 0)
        extra["custom_index_and_mask"] = (int(extra["custom_index_and_mask"]) & 0xFFFFFF) | (0xFF << 24)
        inst = np.concatenate([w.inst, np.array([extra], w.inst.dtype)])
        w.ctx.set_instances(inst)
        model = sr.StackModel(w.ctx.debug_snapshot())
        c = Case((w.verts, w.idx, w.ranges, inst))
        me = len(inst) - 1
        prims = np.array([1, 510])
        refs = np.concatenate([stf.refs(me, prims), stf.refs(me, prims, tss.S_TOP), stf.refs(tss.S_TOP, [9001], me)])
        tris, ok, _ = stf.expand(c.src, refs)
        assert ok.all()
        b = trf.bounds(tris).astype(np.float64)
        peaks = [2 + model.peak(sr.Box(x[0:3], x[4:7]), blas_only=tss.S_TOP)[0] for x in b[:4]]
        peaks_t = [2 + model.peak(TriangleQuery((x[0:3], x[4:7], x[8:11])), blas_only=tss.S_TOP)[0] for x in tris[:4].astype(np.float64)]
        print("modelled entries (sentinel, marker, the deep corridor's BLAS) before the first triangle: boxes %s, triangles %s" % (peaks, peaks_t))
        assert sr.stack2_lds() == tss.STACK2_LDS and min(peaks) >= tss.STACK2_LDS + tss.SINGLE and min(peaks_t) >= tss.STACK2_LDS + tss.SINGLE
        want = c.overlaps(refs)
        assert (want[0][:4] > 1000).all() and (want[0][4:] > 0).all()
        assert (want[1][:2, :, 0] == tss.S_TOP).all()      # (nothing else is near: the others are the deep corridor's squares)
        overlap_modes(w.ctx, c, refs, 0xFF, "corridor")
        nearest_check(w.ctx, c, refs, what="corridor")
        far = stf.refs(me, prims[:1], len(inst) - 2)             # the corridor 1000 units away: the nearest pair across the gap
        ref, _ = nearest_check(w.ctx, c, far, what="corridor, far pair")
        assert (ref["inst"] == len(inst) - 2).all() and (ref["t"] > 500).all()
    finally:
        w.ctx.close()


@pytest.mark.gpu
def test_plumbing(ctx):
    """host form = device form; counting, and the pair form visits less; out= reuse; references written by a kernel queued just before
    the call on a side stream and overwritten right after it; n == 0"""
    import torch
    c = case("close")
    load(ctx, c.parts)
    every = stf.every_triangle(c.sc)
    want = c.overlaps(every)
    cnt, ids, st = ctx.overlap_scene_triangles(every, max_ids=16)
    same((cnt, ids), want, "host form")
    assert st.node_visits == 0 and st.tri_tests == 0 and st.ms_trace_closest > 0 and st.bvh_node_bytes == 32 and st.bvh_tri_bytes == 48
    cnt, ids, st = ctx.overlap_scene_triangles(every.view(api.TRI_REF_DTYPE).reshape(-1), max_ids=16, counting=True)
    same((cnt, ids), want, "host form, counting, TRI_REF_DTYPE records")
    assert st.node_visits > 0 and st.tri_tests >= int(want[0].sum())
    cnt, ids, _ = ctx.overlap_scene_triangles(every, max_ids=3, counts=False)
    assert cnt is None
    same((None, ids), want, "host form without counts", max_ids=3)
    cnt, ids, _ = ctx.overlap_scene_triangles(every, max_ids=0, any=True)
    assert ids is None and np.array_equal(cnt, (want[0] > 0).astype(np.uint32))
    # the same source records against one instance each: the TLAS is not walked
    near = stf.refs(every[:, 0], every[:, 1], (every[:, 0] + 1) % c.n_inst)
    cnt, ids, st_pair = ctx.overlap_scene_triangles(near, max_ids=16, counting=True)
    same((cnt, ids), c.overlaps(near), "host form, pairs")
    assert 0 < st_pair.node_visits < st.node_visits and 0 < st_pair.tri_tests < st.tri_tests
    ref, q_ref = c.nearest(every)
    hh, st = ctx.closest_scene_triangle(every)
    assert hh.tobytes() == ref.tobytes() and st.node_visits == 0 and st.bvh_node_bytes > 0
    hc, q_host, st = ctx.closest_scene_triangle(every, params=True, counting=True)
    assert hc.tobytes() == ref.tobytes() and q_host.tobytes() == q_ref.tobytes() and st.node_visits > 0 and st.tri_tests > 0
    hp, st_pair = ctx.closest_scene_triangle(near, counting=True)
    assert hp.tobytes() == c.nearest(near)[0].tobytes() and 0 < st_pair.node_visits < st.node_visits and 0 < st_pair.tri_tests < st.tri_tests
    # out= reuse
    src = dev(every)
    n = len(every)
    ids_t = torch.empty((n, 16, 2), dtype=torch.int32, device="cuda:0"); cnt_t = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    res = ctx.overlap_scene_triangles_device(src, max_ids=16, out=(ids_t, cnt_t))
    assert res.ids.data_ptr() == ids_t.data_ptr() and res.count.data_ptr() == cnt_t.data_ptr() and isinstance(res, api.BoxOverlaps)
    torch.cuda.synchronize()
    same(res.numpy(), want, "out= reuse")
    hits = torch.empty((n, 5), dtype=torch.int32, device="cuda:0"); attr = torch.empty((n, 8), dtype=torch.int32, device="cuda:0")
    par = torch.empty((n, 2), dtype=torch.float32, device="cuda:0")
    res = ctx.closest_scene_triangle_device(src, attributes=True, params=True, out=(hits, attr, par))
    assert res.hits.data_ptr() == hits.data_ptr() and res.attr.data_ptr() == attr.data_ptr() and res.quv.data_ptr() == par.data_ptr()
    assert res.numpy()[0].tobytes() == ref.tobytes() and res.quv.cpu().numpy().tobytes() == q_ref.tobytes()
    tri_t = torch.empty((n, 12), dtype=torch.float32, device="cuda:0")
    assert ctx.scene_triangles_device(src, out=tri_t).data_ptr() == tri_t.data_ptr()
    torch.cuda.synchronize()
    assert tri_t.cpu().numpy().tobytes() == stf.expand(c.src, every)[0].tobytes()
    with pytest.raises(ValueError):
        ctx.overlap_scene_triangles_device(src, max_ids=16, out=(ids_t[:-1], cnt_t))
    with pytest.raises(ValueError):
        ctx.closest_scene_triangle_device(src, out=(hits[:-1], None))
    with pytest.raises(ValueError):
        ctx.scene_triangles_device(src, out=tri_t[:-1])
    # stream order: the references are made by a kernel behind a slow queue on a side stream, and overwritten right after the calls
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = slow_queue(torch, 12)
        p = (src + (a[0, 0] != a[0, 0]).to(torch.int32) * 0).contiguous()   # made behind the queue, on s
        r1 = ctx.overlap_scene_triangles_device(p, max_ids=16, stream=s)
        r2 = ctx.closest_scene_triangle_device(p, params=True, stream=s)
        r3 = ctx.scene_triangles_device(p, stream=s)
        r4 = ctx.overlap_scene_triangles_device(p, max_ids=0, any=True, stream=s)
        p.zero_()
        i1, c1, h2, q2, t3, c4 = r1.ids.clone(), r1.count.clone(), r2.hits.clone(), r2.quv.clone(), r3.clone(), r4.count.clone()
    s.synchronize()
    same((c1.cpu().numpy().view(np.uint32), i1.cpu().numpy()), want, "stream order")
    assert h2.cpu().numpy().view(HIT_DTYPE).reshape(-1).tobytes() == ref.tobytes() and q2.cpu().numpy().tobytes() == q_ref.tobytes()
    assert t3.cpu().numpy().tobytes() == stf.expand(c.src, every)[0].tobytes()
    assert np.array_equal(c4.cpu().numpy().view(np.uint32), (want[0] > 0).astype(np.uint32))
    # n == 0
    none = torch.empty((0, 4), dtype=torch.int32, device="cuda:0")
    e = ctx.overlap_scene_triangles_device(none, max_ids=4)
    assert e.ids.shape == (0, 4, 2) and e.count.shape == (0,)
    e = ctx.closest_scene_triangle_device(none, attributes=True, params=True)
    assert e.hits.shape == (0, 5) and e.attr.shape == (0, 8) and e.quv.shape == (0, 2)
    assert ctx.scene_triangles_device(none).shape == (0, 12)
    cnt, ids, _ = ctx.overlap_scene_triangles(np.zeros((0, 4), np.int32), max_ids=2)
    assert len(cnt) == 0 and ids.shape == (0, 2, 2) and len(ctx.closest_scene_triangle(np.zeros((0, 4), np.int32))[0]) == 0


@pytest.mark.gpu
def test_frame_in_flight_on_a_second_slot():
    """a frame in flight on a second slot is neither waited for nor changed by the queries on the root: its pixels equal the frame rendered
    alone"""
    import torch
    from tests.test_ray_query import W, H, two_objects
    base = RtContext(0)
    slot = base.frame_slot()
    try:
        sp = two_objects(base)
        slot.set_instances(sp.instances)
        slot.set_uniforms(sp.uniforms)
        before = base.trace(W, H)[0]
        c = Case((sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances))
        refs = stf.every_triangle(c.sc)[::7][:1500]
        src = dev(refs)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        slot.trace_async(W, H)
        with torch.cuda.stream(s):
            slow_queue(torch, 4)
            res = base.overlap_scene_triangles_device(src, max_ids=16, stream=s)
            near = base.closest_scene_triangle_device(src, stream=s)
        during, _ = slot.trace_wait()
        after = base.trace(W, H)[0]
        s.synchronize()
        assert np.array_equal(during.view(np.uint32), before.view(np.uint32)) and np.array_equal(after.view(np.uint32), before.view(np.uint32))
        same(res.numpy(), c.overlaps(refs), "beside frames")
        assert near.numpy()[0].tobytes() == c.nearest(refs)[0].tobytes()
        same(gpu_overlap(slot, refs, max_ids=16), c.overlaps(refs), "on the second slot")
    finally:
        slot.close()
        base.close()


def _raw_o(c, n, refs, cull, flags, k, ids, counts):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_overlap_scene_triangles_device(c.h, n, p(refs), cull, flags, k, p(ids), p(counts), None)


def _raw_n(c, n, refs, cull, hits, attr, par):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_closest_scene_triangle_device(c.h, n, p(refs), cull, p(hits), p(attr), p(par), None)


def _raw_t(c, n, refs, tris):
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731
    return c.L.rt_scene_triangles_device(c.h, n, p(refs), p(tris), None)


@pytest.mark.gpu
def test_error_statuses():
    import torch
    from tests import scenes
    from tests.test_blas_refit import span
    case_c = case("close")
    verts, idx, ranges, inst = case_c.parts
    every = stf.every_triangle(case_c.sc)
    want = case_c.overlaps(every, max_ids=4)
    ref = case_c.nearest(every)[0]
    q = dev(every)
    n = q.shape[0]
    ids = torch.empty((n + 1, 4, 2), dtype=torch.int32, device="cuda:0")
    cnt = torch.empty((n + 1,), dtype=torch.int32, device="cuda:0")
    hits = torch.empty((n + 1, 5), dtype=torch.int32, device="cuda:0")
    attr = torch.empty((n + 1, 8), dtype=torch.int32, device="cuda:0")
    par = torch.empty((n + 1, 2), dtype=torch.float32, device="cuda:0")
    tri = torch.empty((n + 1, 12), dtype=torch.float32, device="cuda:0")
    R_, I_, C_, H_, A_, P_, T_ = (x.data_ptr() for x in (q, ids, cnt, hits, attr, par, tri))
    c = RtContext(0)

    def err(raw, args, code, text):
        assert raw(c, *args) == code, (raw.__name__, args)
        msg = c.L.rt_last_error(c.h).decode()
        assert text in msg, (args, msg)

    def not_ready():
        err(_raw_o, (n, R_, 0xFF, 0, 4, I_, C_), RT_ERR_NOT_READY, "")
        err(_raw_n, (n, R_, 0xFF, H_, 0, 0), RT_ERR_NOT_READY, "")
        err(_raw_t, (n, R_, T_), RT_ERR_NOT_READY, "")

    def ok():
        got = c.overlap_scene_triangles_device(q, max_ids=4).numpy()
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == np.ascontiguousarray(want[1]).tobytes()
        assert c.closest_scene_triangle_device(q).numpy()[0].tobytes() == ref.tobytes()

    try:
        not_ready()                                  # no geometry
        c.upload_geometry(verts, idx, ranges)
        not_ready()                                  # no TLAS
        c.set_instances(inst)
        ok()
        bad = [((0xFFFFFF00, R_, 0xFF, 0, 4, I_, C_), "too many references"), ((0x10000000, R_, 0xFF, 0, 16, I_, C_), "n * max_ids"),
               ((n, R_, 0x100, 0, 4, I_, C_), "cull_mask"), ((n, R_, 0xFF, 0x2, 4, I_, C_), "unknown flag bits"), ((n, R_, 0xFF, 0x80000000, 0, 0, C_), "unknown flag bits"),
               ((n, R_, 0xFF, 0, 17, I_, C_), "max_ids must be 0..16"), ((n, R_, 0xFF, 0, 0, I_, C_), "max_ids 0 counts only"), ((n, R_, 0xFF, 0, 0, I_, 0), "max_ids 0 counts only"),
               ((n, R_, 0xFF, 1, 4, I_, C_), "RT_OVERLAP_ANY needs max_ids 0"), ((n, R_, 0xFF, 1, 0, 0, 0), "neither ids nor counts"),
               ((n, R_, 0xFF, 0, 4, 0, 0), "neither ids nor counts"), ((n, R_, 0xFF, 0, 4, 0, C_), "null id pointer"), ((n, 0, 0xFF, 0, 4, I_, C_), "null reference pointer"),
               ((n, R_ + 4, 0xFF, 0, 4, I_, C_), "aligned"), ((n, R_, 0xFF, 0, 4, I_ + 2, C_), "aligned"), ((n, R_, 0xFF, 0, 4, I_, C_ + 1), "aligned")]
        bad_n = [((0xFFFFFF00, R_, 0xFF, H_, 0, 0), "too many references"), ((n, R_, 0x100, H_, 0, 0), "cull_mask"), ((n, 0, 0xFF, H_, 0, 0), "null reference/hit pointers"),
                 ((n, R_, 0xFF, 0, 0, 0), "null reference/hit pointers"), ((n, R_ + 4, 0xFF, H_, 0, 0), "aligned"), ((n, R_, 0xFF, H_ + 2, 0, 0), "aligned"),
                 ((n, R_, 0xFF, H_, A_ + 4, 0), "aligned"), ((n, R_, 0xFF, H_, 0, P_ + 2), "aligned")]
        bad_t = [((0xFFFFFF00, R_, T_), "too many references"), ((n, 0, T_), "null reference/triangle pointers"), ((n, R_, 0), "null reference/triangle pointers"),
                 ((n, R_ + 4, T_), "aligned"), ((n, R_, T_ + 4), "aligned")]
        host_buf = np.zeros((n + 1, 12), np.float32)
        pinned = torch.zeros((n, 12), dtype=torch.float32).pin_memory()
        for ptr in ((host_buf.ctypes.data + 15) & ~15, pinned.data_ptr()):   # (16-byte aligned: only the memory kind is wrong)
            bad += [((n, ptr, 0xFF, 0, 4, I_, C_), "references, ids and counts must be device memory of the context's GPU"),
                    ((n, R_, 0xFF, 0, 4, ptr, C_), "device memory of the context's GPU"), ((n, R_, 0xFF, 0, 4, I_, ptr), "device memory of the context's GPU")]
            bad_n += [((n, ptr, 0xFF, H_, 0, 0), "device memory of the context's GPU"), ((n, R_, 0xFF, ptr, 0, 0), "device memory of the context's GPU"),
                      ((n, R_, 0xFF, H_, ptr, 0), "device memory of the context's GPU"), ((n, R_, 0xFF, H_, 0, ptr), "device memory of the context's GPU")]
            bad_t += [((n, ptr, T_), "device memory of the context's GPU"), ((n, R_, ptr), "device memory of the context's GPU")]
        for raw, cases, fn in ((_raw_o, bad, "rt_overlap_scene_triangles_device"), (_raw_n, bad_n, "rt_closest_scene_triangle_device"), (_raw_t, bad_t, "rt_scene_triangles_device")):
            for args, text in cases:
                err(raw, args, RT_ERR_INVALID_ARGUMENT, text)
                assert fn in c.L.rt_last_error(c.h).decode()
            ok()
        # 4-byte aligned rows, counts and parameters that are not 8- or 16-byte aligned are fine
        assert _raw_o(c, n, R_, 0xFF, 0, 4, I_ + 4, C_ + 4) == 0
        torch.cuda.synchronize()
        assert ids.view(-1)[1:1 + 8 * n].cpu().numpy().tobytes() == np.ascontiguousarray(want[1]).tobytes() and cnt[1:].cpu().numpy().view(np.uint32).tobytes() == want[0].tobytes()
        assert _raw_n(c, n, R_, 0xFF, H_, 0, P_ + 4) == 0
        out_c = np.zeros(n, np.uint32)
        out_h = np.zeros(n, HIT_DTYPE)
        P = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        assert c.L.rt_overlap_scene_triangles(c.h, n, None, 0xFF, 0, 0, None, P(out_c), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert "null reference pointer" in c.L.rt_last_error(c.h).decode()
        assert c.L.rt_overlap_scene_triangles(c.h, n, P(every), 0x100, 0, 0, None, P(out_c), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_overlap_scene_triangles(c.h, n, P(every), 0xFF, 1, 2, None, P(out_c), 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_overlap_scene_triangles(c.h, n, P(every), 0xFF, 0, 0, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_closest_scene_triangle(c.h, n, None, 0xFF, P(out_h), None, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_closest_scene_triangle(c.h, n, P(every), 0x100, P(out_h), None, 0, None) == RT_ERR_INVALID_ARGUMENT
        ok()
        assert _raw_o(c, 0, 0, 0xFF, 0, 0, 0, C_) == 0 and _raw_n(c, 0, 0, 0xFF, 0, 0, 0) == 0 and _raw_t(c, 0, 0, 0) == 0   # n == 0 needs no pointers
        with pytest.raises(ValueError):
            c.overlap_scene_triangles_device(q.cpu())
        with pytest.raises(ValueError):
            c.overlap_scene_triangles_device(q.to(torch.float32))
        with pytest.raises(ValueError):
            c.closest_scene_triangle_device(torch.zeros((4, 12), dtype=torch.int32, device="cuda:0"))
        with pytest.raises(ValueError):
            c.overlap_scene_triangles_device(q, max_ids=2, any=True)
        with pytest.raises(RtError) as e:
            c.overlap_scene_triangles_device(q, cull_mask=0x1FF)
        assert e.value.code == RT_ERR_INVALID_ARGUMENT
        ok()
        # not ready: a stale TLAS after a BLAS refit
        geom = types.SimpleNamespace(verts=verts, idx=idx, ranges=ranges)
        ff, nf = span(geom, 1)
        v = torch.from_numpy(np.asarray(verts, F)[ff:ff + nf].copy()).to("cuda:0")
        torch.cuda.synchronize()
        c.refit_blas_device(1, v)
        not_ready()
        c.set_instances(inst)
        ok()
        # not ready: a context that holds a frame batch
        sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
        c.set_batch(np.stack([inst, inst]), np.concatenate([sp.uniforms, sp.uniforms]))
        not_ready()
        c.set_instances(inst)
        ok()
    finally:
        c.close()
    # trace_variant != 0 (alt library only: the product refuses the parameter itself)
    a = RtContext(0, variant="alt")
    try:
        a.set_param("blas_builder", 0)
        a.set_param("trace_variant", 1)
        a.upload_geometry(verts, idx, ranges)
        a.set_instances(inst)
        c = a
        err(_raw_o, (n, R_, 0xFF, 0, 4, I_, C_), RT_ERR_INVALID_ARGUMENT, "trace_variant 0")
        err(_raw_n, (n, R_, 0xFF, H_, 0, 0), RT_ERR_INVALID_ARGUMENT, "trace_variant 0")
        err(_raw_t, (n, R_, T_), RT_ERR_INVALID_ARGUMENT, "trace_variant 0")
        a.set_param("trace_variant", 0)
        a.set_instances(inst)
        ok()
    finally:
        a.close()
