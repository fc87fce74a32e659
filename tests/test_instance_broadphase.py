"""rt_instance_pairs*: the broad phase over the scene's instances.  A record (inst, against, r_max) asks which instances' canonical boxes
come within the margin r_max of the source's; the rows are rt_inst_ref records, the input of rt_closest_instances_device and
rt_overlap_instances_device.

tests/instance_broadphase_reference.py holds the reference, numpy straight from the definition of include/rt_api.h.  Offsets and rows are
held byte for byte, whatever the tree.  The CPU part asserts the exports, the kernels' budget, the premises of the GPU tests and, on the
references alone, the guarantee: every pair the narrow phase reports is listed."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import instance_broadphase_reference as ibr
from tests import instance_pair_reference as ipr
from tests.test_instance_pairs import (FLAT, ICO320, MASKED, NOTHING, OCTA, ONE_BIT, VOID, ICO80, case as pair_case, dev, load, median_radius, meshes,
                                       record_list)
from tests.test_ray_query import dev_inst
from tests.test_ray_query_oracle import use_builder
from vulkan_raytracing_amd import RtContext, api, host
from vulkan_raytracing_amd.api import RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
F = np.float32
INSERT_MAX, LDS_TILE = 64, 2048          # RT_LIST_INSERT_MAX, RT_LIST_LDS_TILE (csrc/rt_kernels.h)
SENTINEL = 0x5A5A5A5A


# ---- scenes and their references, computed once -----------------------------------------------------------------------------

def rotation(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def instances_of(mesh, M, t, mask=0xFF):
    """INSTANCE_DTYPE records of meshes `mesh` (n,) with linear parts M (n, 3, 3) and translations t (n, 3)"""
    inst = np.zeros(len(mesh), host.INSTANCE_DTYPE)
    for i in range(len(mesh)):
        inst[i] = host.make_instance(np.concatenate([M[i], t[i][:, None]], axis=1).astype(F).reshape(12), i, int(mesh[i]))
        inst[i]["custom_index_and_mask"] = (int(inst[i]["custom_index_and_mask"]) & 0xFFFFFF) | (mask << 24)
    return inst


def cancel_parts():
    """six octahedra whose mesh lies 1e4 away from its origin and whose translation brings it back, rotated: the row-term magnitude of
    o2w over the mesh is 1e4 while the world coordinates are a few units (the 1e-5 pad of the TLAS leaf box does not cover the rounding
    of such a world vertex, the canonical box's slack does)"""
    verts, idx, ranges = meshes()
    verts = np.array(verts, F, copy=True)
    off = np.array([1.0e4, -1.0e4, 1.0e4])
    p = verts[ranges[OCTA][0]:ranges[OCTA + 1][0]].reshape(-1, 6)
    p[:, :3] = (p[:, :3].astype(np.float64) + off).astype(F)
    rng = np.random.default_rng(97)
    n = 6
    M = np.array([rotation(rng) for _ in range(n)])
    pos = np.array([[1.6 * (i % 3), 1.6 * (i // 3), 0.0] for i in range(n)]) + rng.uniform(-0.3, 0.3, (n, 3))
    t = np.array([pos[i] - M[i] @ off for i in range(n)])
    return verts, idx, ranges, instances_of(np.full(n, OCTA), M, t)


def grid_parts(side=8, seed=5):
    """side^3 small octahedra on a jittered grid of spacing 1, of radius 0.3: with a margin of 0.2 a body lists about ten others"""
    verts, idx, ranges = meshes()
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    n = len(g)
    M = np.array([rotation(rng) * 0.3 for _ in range(n)])
    return verts, idx, ranges, instances_of(np.full(n, OCTA), M, g + rng.uniform(-0.2, 0.2, (n, 3)))


GRID_MARGIN = 0.2


def hub_parts():
    """one icosphere of radius 30 over 2500 small octahedra inside it and 500 far outside: the hub's row is longer than the sort's LDS
    tile, and with a margin of 8 the rows of the inner bodies are longer than what the walk sorts by insertion"""
    verts, idx, ranges = meshes()
    rng = np.random.default_rng(23)
    n_in, n_out = 2500, 500
    d = rng.normal(size=(n_in + n_out, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.concatenate([25.0 * rng.uniform(0, 1, n_in) ** (1 / 3), rng.uniform(100, 200, n_out)])
    M = np.concatenate([[np.eye(3) * 30.0], [rotation(rng) * 0.3 for _ in range(n_in + n_out)]])
    t = np.concatenate([[np.zeros(3)], d * r[:, None]])
    order = rng.permutation(n_in + n_out) + 1                     # (rows are in ascending j: the walk meets them in tree order)
    M[1:], t[1:] = M[order], t[order]
    mesh = np.concatenate([[ICO320], np.full(n_in + n_out, OCTA)])
    return verts, idx, ranges, instances_of(mesh, M, t)


HUB = 0
_CASES = {}
PARTS = {"cancel": cancel_parts, "grid": grid_parts, "hub": hub_parts}


def parts_of(name):
    return pair_case(name).parts if name in ("apart", "close", "tie") else PARTS[name]()


def case(name):
    if name not in _CASES:
        _CASES[name] = ibr.BroadPhase(parts_of(name))
    return _CASES[name]


def narrow(name):
    """the narrow-phase reference (ipr.Pairs) of a scene"""
    if name in ("apart", "close", "tie"):
        return pair_case(name)
    if "pairs_" + name not in _CASES:
        _CASES["pairs_" + name] = ipr.Pairs(parts_of(name))
    return _CASES["pairs_" + name]


def everyone(n, m=0.0, against=-1):
    return ipr.records(np.arange(n), against, m)


def hub_records(c):
    """every body against the others at contact, then the first 100 inner bodies with a margin of 8"""
    return np.concatenate([everyone(c.n_inst), ipr.records(np.arange(1, 101), -1, 8.0)])


def invalid_records(n):
    """inst and against out of range, a negative and a NaN radius, the empty mesh and the void source (scene_parts' numbering)"""
    return ipr.records([-1, n, 2 ** 31 - 1, 0, 0, 0, 0, NOTHING, VOID], [-1, -1, 0, -2, n, 1, 1, -1, -1],
                       np.array([1.0, 2.0, 3.0, 4.0, 5.0, -1.0, np.nan, 6.0, 7.0], F))


def tie_margin():
    """the margin at which Box(1).lo_x - m == Box(0).hi_x in the two-cube scene: 2 - 2^-11 - 2^-13, every value exact"""
    c = case("tie")
    m = F(c.box_lo[1, 0]) - F(c.box_hi[0, 0])
    assert F(c.box_lo[1, 0] - m) == c.box_hi[0, 0] and float(m) == 2.0 - 2.0 ** -11 - 2.0 ** -13
    return m


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

NEW = ("rt_instance_pairs_device", "rt_instance_pairs")


def test_exports_and_abi():
    for name in NEW:
        assert name in api.EXPORTS, name
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^#define RT_INSTANCE_PAIRS_ABOVE 0x1u", hdr, re.M)
    assert re.search(r"^int rt_instance_pairs_device\(rt_ctx\* ctx, size_t n, const void\* d_irefs4, uint32_t cull_mask, uint32_t flags,\s+void\* d_offsets, "
                     r"void\* d_pairs4, size_t capacity, void\* hip_stream\);", hdr, re.M)
    assert re.search(r"^int rt_instance_pairs\(rt_ctx\* ctx, size_t n, const rt_inst_ref\* irefs_host, uint32_t cull_mask, uint32_t flags,\s+uint64_t\* offsets_host, "
                     r"rt_inst_ref\* pairs_host, size_t capacity, int counting, rt_stats\* stats\);", hdr, re.M)
    L = api.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert L.rt_abi_version() == 7
    assert L.rt_instance_pairs_device(None, 0, None, 0xFF, 0, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_instance_pairs(None, 0, None, 0xFF, 0, None, None, 0, 0, None) == RT_ERR_INVALID_ARGUMENT
    for name in ("instance_pairs_device", "instance_pairs"):
        assert hasattr(RtContext, name), name
    assert api.INSTANCE_PAIRS_ABOVE == 1


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_broadphase_kernels_keep_the_record_level_budget(target):
    """the two walks (plain and counting) within the record-level budget (>= 4 waves per SIMD, scratch <= 32 bytes, no spills) in both
    libraries; the box kernel, the scan and the sort without scratch"""
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    for stem in ("k_ipairs_size", "k_ipairs_fill"):
        walk = [(n, r) for n, r in kernels.items() if stem in n]
        assert len(walk) == 2 and sum(stem + "_count" in n for n, _ in walk) == 1, "\n".join(kernels)
        for name, r in walk:
            assert int(r["Occupancy"]) >= 4 and int(r["ScratchSize"]) <= 32 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
    for stem, count in (("k_ipairs_boxes", 1), ("k_ipairs_sort", 1), ("k_list_scan_", 3), ("k_list_sort", 1)):
        ks = [(n, r) for n, r in kernels.items() if stem in n]
        assert len(ks) == count, "\n".join(kernels)
        for name, r in ks:
            assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)


def test_the_resource_report_names_every_earlier_kernel_unchanged():
    """profiles/instance_broadphase.txt records the report of both libraries before and after the broad-phase kernels: every kernel of the
    earlier report is in the later one with the same figures, k_list_sort (whose body became a template) among them"""
    text = open(os.path.join(ROOT, "profiles", "instance_broadphase.txt")).read()
    for lib in ("product", "alt"):
        before = dict(re.findall(r"^before %s (\S+) (.*)$" % lib, text, re.M))
        after = dict(re.findall(r"^after %s (\S+) (.*)$" % lib, text, re.M))
        assert len(before) >= 80 and all(after.get(k) == v for k, v in before.items()), lib
        assert sum("k_ipairs_" in k for k in after) == 6 and not any("k_ipairs_" in k for k in before)
        assert any("k_list_sort" in k for k in before)


def test_the_scenes_cross_the_boundaries():
    """the premises of the GPU tests, on the reference alone"""
    a, c = case("apart"), case("close")
    assert a.n_inst == 12 and not a.source[NOTHING] and not a.source[VOID] and a.source[MASKED] and a.source[FLAT] and a.mask[MASKED] == 0 and a.mask[VOID] == 0
    lens = lambda o: np.diff(o.astype(np.int64))   # noqa: E731
    # rows of length 0 and 1
    o, p = a.rows(everyone(a.n_inst))
    assert (lens(o) == 0).sum() >= 3 and (lens(c.rows(everyone(c.n_inst))[0]) >= 5).any()
    o1, p1 = a.rows(record_list(a.n_inst))
    assert set(lens(o1)[record_list(a.n_inst)[:, 1] >= 0].tolist()) == {0, 1}
    # beyond RT_LIST_INSERT_MAX and beyond the sort's LDS tile: the hub scene
    h = case("hub")
    assert h.n_inst == 3001 and h.source.all()
    recs = hub_records(h)
    oh, ph = h.rows(recs)
    lh = lens(oh)
    print("hub: row of the hub %d, rows of the margin records %d .. %d, %d rows longer than %d, total %d" %
          (lh[HUB], lh[h.n_inst:].min(), lh[h.n_inst:].max(), (lh > INSERT_MAX).sum(), INSERT_MAX, oh[-1]))
    assert lh[HUB] >= LDS_TILE + 1 and (lh[h.n_inst:] >= INSERT_MAX + 1).sum() >= 50 and (lh == 1).sum() > 100 and (lh == 0).sum() > 100
    assert ((lh > 1) & (lh <= INSERT_MAX)).sum() > 100
    # the records fall on and off the edges of the walk's 64-record chunks: long rows in the first and in inner lanes of a chunk, a last
    # chunk that is not full, and (the grid) a call of whole chunks
    long_at = np.nonzero(lh > INSERT_MAX)[0]
    assert (long_at % 64 == 0).any() and (long_at % 64 != 0).any() and len(recs) % 64 != 0 and case("grid").n_inst % 64 == 0
    # ... and the rows on and off multiples of 64 entries
    assert (oh[1:-1] % 64 == 0).any() and (oh[1:-1] % 64 != 0).any()
    # the grid: about ten neighbours
    g = case("grid")
    lg = lens(g.rows(everyone(g.n_inst, GRID_MARGIN))[0])
    print("grid: %d bodies, rows %d .. %d, mean %.2f" % (g.n_inst, lg.min(), lg.max(), lg.mean()))
    assert 6 <= lg.mean() <= 14
    # ABOVE halves the symmetric pairs
    for s, m in ((g, GRID_MARGIN), (h, 0.0), (c, 0.0)):
        full, _ = s.rows(everyone(s.n_inst, m))
        half, hp = s.rows(everyone(s.n_inst, m), above=True)
        sym = {(int(i), int(j)) for i, j in s.rows(everyone(s.n_inst, m))[1][:, :2]}
        if all((j, i) in sym for i, j in sym):
            assert int(full[-1]) == 2 * int(half[-1])
        assert (hp[:, 1] > hp[:, 0]).all() and {(int(i), int(j)) for i, j in hp[:, :2]} == {(i, j) for i, j in sym if j > i}
    assert int(g.rows(everyone(g.n_inst, GRID_MARGIN))[0][-1]) == 2 * int(g.rows(everyone(g.n_inst, GRID_MARGIN), above=True)[0][-1]) > 0
    # the cull mask takes candidates out, never sources
    one = a.rows(everyone(a.n_inst, np.inf), ONE_BIT)[0]
    full = a.rows(everyone(a.n_inst, np.inf))[0]
    assert 0 < one[-1] < full[-1] and a.rows(everyone(a.n_inst, np.inf), 0)[0][-1] == 0
    assert len(a.row(MASKED, -1, np.inf)) > 0 and MASKED not in a.rows(everyone(a.n_inst, np.inf))[1][:, 1]
    # the cancellation scene: the slack is that of the 1e4 terms
    k = case("cancel")
    assert (k.mw > 1.0e4).all() and (np.abs(k.box_lo) < 10).all() and ((k.box_hi - k.box_lo) > 2.0).all()


def test_the_closed_test_has_a_tie_and_the_next_margin_below_drops_it():
    c = case("tie")
    m = tie_margin()
    below = np.nextafter(m, F(0))
    assert c.row(1, 0, m).tolist() == [0] and c.row(1, -1, m).tolist() == [0] and c.row(1, 0, below).tolist() == [] and c.row(1, -1, below).tolist() == []
    assert c.row(0, 0, 0.0).tolist() == [0] and c.row(0, -1, 0.0).tolist() == []      # (against == inst is not special)


@pytest.mark.parametrize("name", ["apart", "close", "cancel"])
def test_every_pair_the_narrow_phase_reports_is_listed(name):
    """the guarantee, on the references alone: for margins 0, the median distance and +inf, every (i, j) for which ipr's overlaps counts
    a pair, or ipr's nearest returns a hit within the margin, has j in the row of (i, -1, m) under the same cull mask"""
    bp, np_ = case(name), narrow(name)
    n = bp.n_inst
    src, dst = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    med = median_radius(np_, ipr.records(src, dst, np.inf))
    checked = 0
    for cull in (0xFF, ONE_BIT):
        touching = np_.overlaps(ipr.records(src, dst), cull)[0] > 0
        for m in (F(0.0), med, F(np.inf)):
            near = np_.nearest(ipr.records(src, dst, m), cull)[0]["inst"] >= 0
            rows = [set(bp.row(i, -1, m, cull).tolist()) for i in range(n)]
            for i, j, t, h in zip(src, dst, touching, near):
                if t or h:
                    checked += 1
                    assert int(j) in rows[int(i)], (name, int(i), int(j), float(m), cull, bool(t), bool(h))
    assert checked > 20, checked


# ---- GPU helpers ------------------------------------------------------------------------------------------------------------------

def gpu_rows(ctx, irefs, cull=0xFF, above=False, capacity=None, extra=7):
    """(offsets uint64 (n + 1,), the whole pair buffer int32 (capacity + extra, 4)): the buffer starts as SENTINEL"""
    import torch
    n = len(irefs)
    d = irefs if isinstance(irefs, torch.Tensor) else dev(irefs)
    offsets = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda:0")
    buf = torch.full((capacity + extra, 4), SENTINEL, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    res = ctx.instance_pairs_device(d, cull_mask=cull, above=above, out=(offsets, buf[:capacity] if capacity else None))
    torch.cuda.synchronize()
    assert res.offsets is offsets and (capacity == 0) == (res.pairs is None)
    return offsets.cpu().numpy().view(np.uint64), buf.cpu().numpy()


def check(ctx, bp, irefs, cull=0xFF, above=False, what=""):
    """the offsets and, with exactly the total as the capacity, the rows against the reference; nothing beyond them written; twice the
    same bytes"""
    ro, rp = bp.rows(irefs, cull, above)
    T = int(ro[-1])
    got = gpu_rows(ctx, irefs, cull, above, T)
    again = gpu_rows(ctx, irefs, cull, above, T)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes(), what + ": two runs differ"
    o, p = got
    if o.tobytes() != ro.tobytes():
        bad = np.nonzero(np.diff(o.astype(np.int64)) != np.diff(ro.astype(np.int64)))[0]
        raise AssertionError("%s: %d rows differ in length, first %d: record %s gpu %d expected %d" %
                             (what, len(bad), bad[0], irefs[bad[0]], o[bad[0] + 1] - o[bad[0]], ro[bad[0] + 1] - ro[bad[0]]))
    if p[:T].tobytes() != rp.tobytes():
        bad = np.nonzero((p[:T] != rp).any(axis=1))[0]
        raise AssertionError("%s: %d entries differ, first %d: gpu %s expected %s" % (what, len(bad), bad[0], p[bad[0]], rp[bad[0]]))
    assert (p[T:] == SENTINEL).all(), what
    return ro, rp


def all_checks(ctx, bp, what, margins=(0.0, 0.7, np.inf)):
    n = bp.n_inst
    for m in margins:
        check(ctx, bp, everyone(n, m), what="%s, margin %g" % (what, m))
    check(ctx, bp, everyone(n, margins[1]), above=True, what=what + ", above")
    check(ctx, bp, everyone(n, np.inf), ONE_BIT, what=what + ", one bit")
    check(ctx, bp, record_list(n, margins[1]), what=what + ", every ordered pair")


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["apart", "close"])
def test_rows(ctx, layout):
    """every body against the others and every ordered pair (against >= 0, against == inst among them), margins 0, 0.7 and +inf, cull
    masks 0xFF, one bit and 0, ABOVE, and invalid records among valid ones"""
    bp = case(layout)
    load(ctx, bp.parts)
    all_checks(ctx, bp, layout)
    n = bp.n_inst
    check(ctx, bp, everyone(n, np.inf), 0x00, what=layout + ", cull 0")
    check(ctx, bp, record_list(n, 0.7), ONE_BIT, above=True, what=layout + ", every ordered pair, one bit, above")
    good = record_list(n, np.inf)[::5]
    bad = invalid_records(n)
    mixed = np.concatenate([bad[:4], good[:10], bad[4:], good[10:]])
    ro, rp = check(ctx, bp, mixed, what=layout + ", mixed")
    lens = np.diff(ro.astype(np.int64))
    assert (lens[:4] == 0).all() and (lens[14:14 + len(bad) - 4] == 0).all() and lens.sum() > 10
    ro, _ = check(ctx, bp, bad, what=layout + ", invalid only")
    assert ro[-1] == 0


@pytest.mark.gpu
def test_ties_and_the_cancellation_scene(ctx):
    c = case("tie")
    load(ctx, c.parts)
    m = tie_margin()
    recs = ipr.records([1, 1, 1, 1, 0, 0, 0], [0, -1, 0, -1, 0, -1, 1], np.array([m, m, np.nextafter(m, F(0)), np.nextafter(m, F(0)), 0.0, 0.0, np.inf], F))
    ro, rp = check(ctx, c, recs, what="tie")
    assert np.diff(ro.astype(np.int64)).tolist() == [1, 1, 0, 0, 1, 0, 1]
    k = case("cancel")
    load(ctx, k.parts)
    all_checks(ctx, k, "cancel", margins=(0.0, 0.2, np.inf))
    load(ctx, k.parts, device=True)
    all_checks(ctx, k, "cancel, device TLAS", margins=(0.0, 0.2, np.inf))


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["rt_set_instances", "rt_set_instances_device"])
def test_long_rows_and_the_sort(device):
    """the hub scene: rows of 0 and 1, rows kept sorted by insertion, rows beyond RT_LIST_INSERT_MAX (sorted in LDS) and the hub's row
    beyond RT_LIST_LDS_TILE (merged through global memory); ABOVE; and the grid scene"""
    h = case("hub")
    ctx = RtContext(0)
    try:
        load(ctx, h.parts, device)
        recs = hub_records(h)
        ro, _ = check(ctx, h, recs, what="hub")
        assert (ro[HUB + 1] - ro[HUB]) > LDS_TILE
        check(ctx, h, recs, above=True, what="hub, above")
        check(ctx, h, ipr.records([HUB, HUB, 5], [-1, -1, -1], np.array([0.0, np.inf, np.inf], F)), what="hub, three long rows")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["rt_set_instances", "rt_set_instances_device"])
def test_tlas_producers_and_an_update(device):
    a, c = case("apart"), case("close")
    ctx = RtContext(0)
    try:
        load(ctx, a.parts, device)
        all_checks(ctx, a, "built")
        load(ctx, c.parts, device, update=True)       # (the bodies move: the boxes follow the records, whatever the refitted tree)
        all_checks(ctx, c, "updated")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "1", "2"])
def test_blas_builders_and_a_refit(builder, monkeypatch):
    """the same bytes whatever builder made the meshes' trees (the box comes from the exact bounds, not from a quantisation frame), and
    after rt_refit_blas_device, which changes two meshes' bounds, and a TLAS update those of the reference over the new vertices"""
    import torch
    c = case("close")
    verts, idx, ranges, inst = c.parts
    ctx = RtContext(0)
    try:
        use_builder(ctx, builder, monkeypatch)
        load(ctx, c.parts, device=True)
        all_checks(ctx, c, "builder " + builder)
        v2 = np.array(verts, F, copy=True)
        for mesh in (OCTA, ICO80):
            ff, n = ranges[mesh][0], ranges[mesh + 1][0] - ranges[mesh][0]
            p = v2[ff:ff + n].reshape(-1, 6)
            p[:, :3] *= (np.array([1.3, 0.8, 1.1], F) + (0.1 * np.sin(5.0 * p[:, [1, 2, 0]])).astype(F))   # (the bounds change)
            torch.cuda.synchronize()
            ctx.refit_blas_device(mesh, dev(p))
        torch.cuda.synchronize()
        ctx.set_instances_device(dev_inst(inst), update=True)
        if "refit" not in _CASES:
            _CASES["refit"] = ibr.BroadPhase((v2, idx, ranges, inst))
        new = case("refit")
        assert new.box_lo.tobytes() != c.box_lo.tobytes()
        all_checks(ctx, new, "refit, builder " + builder)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_capacity_and_untouched_bytes(ctx):
    """capacity T, T - 1, exactly at a row boundary, one short of it and 0: a row is written if and only if it ends within the capacity,
    and no other byte of the buffer changes"""
    bp = case("close")
    load(ctx, bp.parts)
    recs = np.concatenate([everyone(bp.n_inst, 0.7), record_list(bp.n_inst, 0.7)[::3]])
    ro, rp = bp.rows(recs)
    T = int(ro[-1])
    ends = ro[1:][np.diff(ro.astype(np.int64)) > 0].astype(np.int64)
    mid = int(ends[len(ends) // 2])
    assert T > 40 and 0 < mid < T
    for cap in (T, T - 1, mid, mid - 1, 1, T + 5):
        o, p = gpu_rows(ctx, recs, capacity=cap)
        assert o.tobytes() == ro.tobytes(), cap
        want = np.concatenate([ibr.written(ro, rp, cap, np.full((cap, 4), SENTINEL, np.int32)), np.full((7, 4), SENTINEL, np.int32)])
        assert p.tobytes() == want.tobytes(), (cap, np.nonzero((p != want).any(axis=1))[0][:5])
    o, p = gpu_rows(ctx, recs, capacity=0)
    assert o.tobytes() == ro.tobytes() and (p == SENTINEL).all()
    # capacity=None: the wrapper sizes the buffer itself
    import torch
    res = ctx.instance_pairs_device(dev(recs))
    offsets, pairs, total = res
    torch.cuda.synchronize()
    assert int(total) == T and tuple(pairs.shape) == (T, 4) and pairs.cpu().numpy().tobytes() == rp.tobytes()
    assert res.numpy()[0].tobytes() == ro.tobytes()


@pytest.mark.gpu
def test_records_from_a_kernel_on_the_same_stream(ctx):
    """the records are written by torch kernels on the stream of the call immediately before it, with no host synchronisation between
    them; a call that read early would see the invalid records the buffer held"""
    import torch
    bp = case("grid")
    load(ctx, bp.parts, device=True)
    n = bp.n_inst
    want = everyone(n, GRID_MARGIN)
    ro, rp = bp.rows(want)
    T = int(ro[-1])
    s = torch.cuda.Stream()
    d = torch.full((n, 4), -1, dtype=torch.int32, device="cuda:0")
    offsets = torch.zeros((n + 1,), dtype=torch.int64, device="cuda:0")
    pairs = torch.full((T, 4), SENTINEL, dtype=torch.int32, device="cuda:0")
    mbits = int(np.array([GRID_MARGIN], F).view(np.int32)[0])
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for _ in range(20):                                   # (work in front of the records, so that the stream is behind the host)
            d.copy_(torch.full((n, 4), -1, dtype=torch.int32, device="cuda:0"))
        d[:, 0] = torch.arange(n, dtype=torch.int32, device="cuda:0")
        d[:, 1] = -1
        d[:, 2] = mbits
        d[:, 3] = 0
        ctx.instance_pairs_device(d, out=(offsets, pairs), stream=s)
    s.synchronize()
    assert d.cpu().numpy().tobytes() == want.tobytes()
    assert offsets.cpu().numpy().view(np.uint64).tobytes() == ro.tobytes() and pairs.cpu().numpy().tobytes() == rp.tobytes()


@pytest.mark.gpu
def test_host_form_and_counting(ctx):
    """the host form equals the device form; with counting the TLAS node visits of the grid scene are well below n x TLAS nodes (a body
    lists about ten of 512: the walk opens a few dozen nodes per record and walk, the TLAS has 511; a quarter of n x nodes for the two
    walks together is a loose bound on that, an inequality and not a measurement)"""
    bp = case("grid")
    load(ctx, bp.parts)
    n = bp.n_inst
    recs = everyone(n, GRID_MARGIN)
    ro, rp = check(ctx, bp, recs, what="grid")
    T = int(ro[-1])
    o, p, st = ctx.instance_pairs(recs)
    assert o.tobytes() == ro.tobytes() and p.tobytes() == rp.tobytes() and st.node_visits == 0 and st.tri_tests == 0 and st.ms_trace_closest > 0
    o, p, st = ctx.instance_pairs(recs.view(api.INST_REF_DTYPE).reshape(-1), capacity=T, counting=True)
    assert o.tobytes() == ro.tobytes() and p.tobytes() == rp.tobytes()
    print("grid: %d node visits and %d box tests for %d records, %d listed" % (st.node_visits, st.tri_tests, n, T))
    assert 0 < st.node_visits < n * (n - 1) // 4 and 2 * T <= st.tri_tests < n * n // 4
    o, p, st1 = ctx.instance_pairs(recs, capacity=0, counting=True)
    assert o.tobytes() == ro.tobytes() and p is None and 0 < st1.node_visits < st.node_visits
    # rows that do not fit stay as they were; above and the cull mask reach the host form
    o, p, _ = ctx.instance_pairs(recs, capacity=T - 1)
    assert p.tobytes() == ibr.written(ro, rp, T - 1, np.zeros((T - 1, 4), np.int32)).tobytes()
    o, p, _ = ctx.instance_pairs(recs, above=True)
    ho, hp = bp.rows(recs, above=True)
    assert o.tobytes() == ho.tobytes() and p.tobytes() == hp.tobytes()
    o, p, _ = ctx.instance_pairs(recs, cull_mask=0)
    assert o[-1] == 0 and p is None


@pytest.mark.gpu
def test_error_returns_and_an_empty_call():
    import torch
    c = case("tie")
    ctx = RtContext(0)
    try:
        L, h = ctx.L, ctx.h
        vp = ctypes.c_void_p
        n = 4
        recs = dev(ipr.records([0, 1, 0, 1], [1, 0, -1, -1], np.inf))
        offsets = torch.zeros((n + 2,), dtype=torch.int64, device="cuda:0")
        pairs = torch.zeros((16, 4), dtype=torch.int32, device="cuda:0")
        R, O, P = recs.data_ptr(), offsets.data_ptr(), pairs.data_ptr()
        p = lambda x: vp(x) if x else None   # noqa: E731
        call = lambda n_, r, o, pp, cap, flags=0, mask=0xFF: L.rt_instance_pairs_device(h, n_, p(r), mask, flags, p(o), p(pp), cap, None)   # noqa: E731
        assert call(n, R, O, P, 16) == RT_ERR_NOT_READY
        verts, idx, ranges, inst = c.parts
        ctx.upload_geometry(verts, idx, ranges)
        assert call(n, R, O, P, 16) == RT_ERR_NOT_READY
        ctx.set_instances(inst)
        assert call(n, R, O, P, 16) == 0
        torch.cuda.synchronize()
        ro, rp = c.rows(recs.cpu().numpy())
        assert offsets.cpu().numpy()[:n + 1].view(np.uint64).tobytes() == ro.tobytes() and pairs.cpu().numpy()[:int(ro[-1])].tobytes() == rp.tobytes()
        assert ro[-1] == 4 and (pairs[4:] == 0).all() and offsets[n + 1] == 0
        # NULL and misaligned pointers, memory of the host
        for args in ((0, O, P, 16), (R, 0, P, 16), (R + 8, O, P, 16), (R, O + 4, P, 16), (R, O, P + 8, 16), (R, O, P + 4, 15)):
            assert call(n, *args) == RT_ERR_INVALID_ARGUMENT, args
        host_mem = np.zeros(64, np.int64)
        assert call(n, host_mem.ctypes.data, O, P, 16) == RT_ERR_INVALID_ARGUMENT and call(n, R, host_mem.ctypes.data, P, 16) == RT_ERR_INVALID_ARGUMENT
        # pairs and capacity go together; the sizes; the flags; the cull mask
        assert call(n, R, O, 0, 16) == RT_ERR_INVALID_ARGUMENT and call(n, R, O, P, 0) == RT_ERR_INVALID_ARGUMENT and call(n, R, O, 0, 0) == 0
        assert call(0xFFFFFF00, R, O, P, 16) == RT_ERR_INVALID_ARGUMENT and call(n, R, O, P, 0xFFFFFF00) == RT_ERR_INVALID_ARGUMENT
        assert call(n, R, O, P, 16, flags=2) == RT_ERR_INVALID_ARGUMENT and call(n, R, O, P, 16, flags=0x80000001) == RT_ERR_INVALID_ARGUMENT
        assert call(n, R, O, P, 16, flags=api.INSTANCE_PAIRS_ABOVE) == 0
        assert call(n, R, O, P, 16, mask=0x100) == RT_ERR_INVALID_ARGUMENT
        st = api.RtStats()
        assert L.rt_instance_pairs(h, n, None, 0xFF, 0, vp(host_mem.ctypes.data), None, 0, 0, ctypes.byref(st)) == RT_ERR_INVALID_ARGUMENT
        assert L.rt_instance_pairs(h, n, vp(host_mem.ctypes.data), 0xFF, 0, None, None, 0, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert L.rt_instance_pairs(h, n, vp(host_mem.ctypes.data), 0xFF, 0, vp(host_mem.ctypes.data), None, 4, 0, None) == RT_ERR_INVALID_ARGUMENT
        with pytest.raises(RtError):
            ctx.instance_pairs(ipr.records([0], [1]), cull_mask=0x100)
        # n == 0: nothing is enqueued, nothing is written
        torch.cuda.synchronize()
        offsets.fill_(77); pairs.fill_(77)
        assert call(0, R, O, P, 16) == 0 and call(0, 0, 0, 0, 0) == 0
        torch.cuda.synchronize()
        assert (offsets == 77).all() and (pairs == 77).all()
        empty = ctx.instance_pairs_device(dev(np.zeros((0, 4), np.int32)))
        assert tuple(empty.offsets.shape) == (1,) and int(empty.total) == 0 and empty.pairs is None
        o, pp, _ = ctx.instance_pairs(np.zeros((0, 4), np.int32))
        assert o.tolist() == [0] and pp is None
    finally:
        ctx.close()
    a = RtContext(0, variant="alt")   # trace_variant != 0 (alt library only: the product refuses the parameter itself)
    try:
        a.set_param("blas_builder", 0)
        a.set_param("trace_variant", 1)
        a.upload_geometry(verts, idx, ranges)
        a.set_instances(inst)
        args = (n, vp(R), 0xFF, 0, vp(O), vp(P), 16, None)
        assert a.L.rt_instance_pairs_device(a.h, *args) == RT_ERR_INVALID_ARGUMENT and "trace_variant 0" in a.L.rt_last_error(a.h).decode()
        a.set_param("trace_variant", 0)
        a.set_instances(inst)
        assert a.L.rt_instance_pairs_device(a.h, *args) == 0
        torch.cuda.synchronize()
    finally:
        a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["close", "apart"])
def test_the_rows_feed_the_narrow_phase(ctx, layout):
    """the rows, passed on as they are, give ipr's answers for those pairs; on the close scene the per-pair counts of row i sum to the
    count of (i, -1), and (both scenes) every other body is apart from i: the guarantee on the device"""
    import torch
    bp, nr = case(layout), narrow(layout)
    load(ctx, bp.parts)
    n = bp.n_inst
    m = F(0.0) if layout == "close" else median_radius(nr, record_list(n))
    recs = everyone(n, m)
    T = int(bp.rows(recs)[0][-1])
    offsets, pairs, total = ctx.instance_pairs_device(dev(recs), capacity=T + 3)
    assert int(total) == T
    rows = pairs[:T]
    count, _ = ctx.overlap_instances_device(rows)
    res = ctx.closest_instances_device(rows)
    alone, _ = ctx.overlap_instances_device(dev(recs))
    near_alone = ctx.closest_instances_device(dev(recs))
    torch.cuda.synchronize()
    rows_h = rows.cpu().numpy()
    o = offsets.cpu().numpy()
    want_c, _ = nr.overlaps(rows_h)
    want_h, want_src, _, _ = nr.nearest(rows_h)
    assert count.cpu().numpy().view(np.uint64).tobytes() == want_c.tobytes()
    assert res.numpy()[0].tobytes() == want_h.tobytes() and res.src_prim.cpu().numpy().tobytes() == want_src.tobytes()
    sums = np.array([int(want_c[int(o[i]):int(o[i + 1])].sum()) for i in range(n)], np.uint64)
    assert sums.tobytes() == alone.cpu().numpy().view(np.uint64).tobytes()
    if layout == "close":
        assert (sums > 0).sum() >= 5
    # the nearest body of i within the margin is in row i
    ha = near_alone.numpy()[0]
    for i in np.nonzero(ha["inst"] >= 0)[0]:
        assert ha["inst"][i] in rows_h[int(o[i]):int(o[i + 1]), 1], i
