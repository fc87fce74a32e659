"""rt_closest_instances* and rt_overlap_instances*: the two by-reference triangle queries per pair of bodies.  A record (inst, against,
r_max) stands for every triangle of its source instance; the answer is the reduction of the per-triangle answers.

tests/instance_pair_reference.py holds the reference, built from scene_triangle_reference and triangle_distance_reference: the canonical
d2 of every (source triangle, candidate) pair, the minimum by (d2, p), and that call's record for the winner.  Everything is held byte for
byte, whatever the tree and whatever order the walk's atomics arrive in.  The CPU part asserts the premises of the GPU tests on the
reference alone, the exports, and the kernels' register budget."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import instance_pair_reference as ipr
from tests.test_ray_query import dev_inst
from tests.test_ray_query_oracle import small_meshes, use_builder
from vulkan_raytracing_amd import RtContext, api, host
from vulkan_raytracing_amd.api import HIT_DTYPE, RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
F = np.float32
OCTA, SOUP, ICO80, ICO320, EMPTY = range(5)
MASKED, VOID, FLAT, NOTHING, BIG = 4, 5, 6, 7, 3   # the instances with mask 0, a NaN transform, a singular transform, the empty mesh, the 320-triangle mesh
ONE_BIT = 0x02


# ---- scenes and their references, computed once -----------------------------------------------------------------------------

def icosphere(levels):
    """the unit icosahedron subdivided `levels` times: 20 * 4^levels outward triangles"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, g = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v, F), np.array(f, np.uint32)


def meshes():
    """mesh 0: the octahedron (8), 1: small_scene's soup (12), 2: an icosphere of 80, 3: one of 320, 4: a mesh without triangles"""
    verts, idx, ranges = small_meshes(157)
    verts, idx, ranges = [np.asarray(verts, F)], [np.asarray(idx, np.uint32)], list(ranges)
    for levels in (1, 2):
        p, f = icosphere(levels)
        ranges.append((sum(len(x) for x in verts), sum(len(x) for x in idx), len(f)))
        verts.append(np.concatenate([p, p], axis=1).astype(F).reshape(-1))
        idx.append(f.reshape(-1))
    ranges.append((sum(len(x) for x in verts), sum(len(x) for x in idx), 0))
    return np.concatenate(verts), np.concatenate(idx), ranges


def scene_parts(name):
    """twelve instances on a 3 x 2 x 2 grid: sheared, mirrored and scaled ones, MASKED with mask 0, VOID with a NaN in its transform, FLAT
    flattened (singular), NOTHING of the empty mesh.  `apart`: 4 units between the centres; `close`: the translations x 0.3, the bodies
    interpenetrate"""
    verts, idx, ranges = meshes()
    rng = np.random.default_rng(411)
    which = [OCTA, SOUP, ICO80, ICO320, OCTA, SOUP, ICO80, EMPTY, OCTA, SOUP, ICO80, OCTA]
    inst = np.zeros(len(which), host.INSTANCE_DTYPE)
    for i, mesh in enumerate(which):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        M = R @ np.diag(rng.uniform(0.7, 1.3, 3))
        if i % 3 == 1:
            M = M @ np.array([[1, rng.uniform(-0.5, 0.5), 0], [0, 1, rng.uniform(-0.5, 0.5)], [0, 0, 1]])
        if i % 4 == 2:
            M = M @ np.diag([-1.0, 1.0, 1.0])
        if i == FLAT:
            M[:, 2] = 0.0
        g = np.array([i % 3, (i // 3) % 2, i // 6], np.float64) - (1.0, 0.5, 0.5)
        t = (g * 4.0 + rng.uniform(-0.4, 0.4, 3)) * (0.3 if name == "close" else 1.0)
        inst[i] = host.make_instance(np.concatenate([M, t[:, None]], axis=1).astype(F).reshape(12), 7 * i + mesh, mesh)
        mask = 0 if i == MASKED else (1 << (i % 3)) | (0x80 if i % 2 else 0)
        inst[i]["custom_index_and_mask"] = (int(inst[i]["custom_index_and_mask"]) & 0xFFFFFF) | (mask << 24)
    inst[VOID]["transform"][5] = np.nan
    return verts, idx, ranges, inst


def tie_parts():
    """two axis-aligned unit cubes [0, 1]^3, the second translated by exactly 3.0 along x: the gap is 2.0 and every value is exact"""
    p = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], F)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.uint32)
    verts = np.concatenate([p, p - F(0.5)], axis=1).astype(F).reshape(-1)
    inst = np.zeros(2, host.INSTANCE_DTYPE)
    for i in range(2):
        inst[i] = host.make_instance(np.array([1, 0, 0, 3.0 * i, 0, 1, 0, 0, 0, 0, 1, 0], F), i, 0)
        inst[i]["custom_index_and_mask"] = (int(inst[i]["custom_index_and_mask"]) & 0xFFFFFF) | (0xFF << 24)
    return verts, f.reshape(-1), [(0, 0, 12)], inst


_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = ipr.Pairs(tie_parts() if name == "tie" else scene_parts(name))
    return _CASES[name]


def record_list(n_inst, r_max=np.inf):
    """every ordered pair (a, b), a == b included, and every a against the others; the 320-triangle source first, so that record
    boundaries fall on the edges of the walk's 64-item chunks as well as inside them"""
    order = [BIG] + [a for a in range(n_inst) if a != BIG]
    return ipr.records(np.repeat(order, n_inst + 1), np.tile(np.arange(-1, n_inst), n_inst), r_max)


def with_radius(irefs, r):
    out = irefs.copy()
    out[:, 2] = np.full(len(out), r, F).view(np.int32)
    return out


def median_radius(c, irefs):
    h = c.nearest(irefs)[0]
    return F(np.median(h["t"][h["inst"] >= 0]))


def invalid_records(c):
    """inst and against out of range, a negative and a NaN radius; and, valid but empty, the empty mesh and the void source"""
    n = c.n_inst
    return ipr.records([-1, n, 2 ** 31 - 1, 0, 0, 0, 0, NOTHING, VOID], [-1, -1, 0, -2, n, 1, 1, -1, -1],
                       np.array([1.0, 2.0, 3.0, 4.0, 5.0, -1.0, np.nan, 6.0, 7.0], F))


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

NEW = ("rt_closest_instances_device", "rt_closest_instances", "rt_overlap_instances_device", "rt_overlap_instances")


def test_exports_struct_and_abi():
    for name in NEW:
        assert name in api.EXPORTS, name
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"typedef struct rt_inst_ref \{\s+int32_t inst;[^}]*int32_t against;[^}]*float\s+r_max;[^}]*uint32_t reserved;[^}]*\} rt_inst_ref;", hdr)
    assert re.search(r"^int rt_closest_instances_device\(rt_ctx\* ctx, size_t n, const void\* d_irefs4, uint32_t cull_mask,\s+void\* d_hits, void\* d_src_prims, "
                     r"void\* d_attr, void\* d_params, void\* hip_stream\);", hdr, re.M)
    assert re.search(r"^int rt_overlap_instances_device\(rt_ctx\* ctx, size_t n, const void\* d_irefs4, uint32_t cull_mask, uint32_t flags,\s+void\* d_counts64, "
                     r"void\* d_first4, void\* hip_stream\);", hdr, re.M)
    L = api.lib()
    for name in NEW:
        assert hasattr(L, name), name
    assert L.rt_abi_version() == 7
    assert L.rt_closest_instances_device(None, 0, None, 0xFF, None, None, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_closest_instances(None, 0, None, 0xFF, None, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_overlap_instances_device(None, 0, None, 0xFF, 0, None, None, None) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_overlap_instances(None, 0, None, 0xFF, 0, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
    for name in ("closest_instances_device", "closest_instances", "overlap_instances_device", "overlap_instances"):
        assert hasattr(RtContext, name), name
    assert api.INST_REF_DTYPE.itemsize == 16 and api.INST_REF_DTYPE.names == ("inst", "against", "r_max", "reserved")
    r = api.instance_refs([3, 4], against=[-1, 2], r_max=np.array([0.5, np.nan], F))
    assert np.array_equal(r, ipr.records([3, 4], [-1, 2], np.array([0.5, np.nan], F))) and r.dtype == np.int32 and r.shape == (2, 4)
    v = r.view(api.INST_REF_DTYPE).reshape(-1)
    assert v["inst"].tolist() == [3, 4] and v["against"].tolist() == [-1, 2] and (v["reserved"] == 0).all()


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_pair_kernels_keep_the_record_level_budget(target):
    """the four walks within the record-level budget (>= 4 waves per SIMD, scratch <= 32 bytes, no spills) in both libraries;
    k_pairs_plan and k_pairs_refs without scratch"""
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    for stem in ("k_pairs_nearest", "k_pairs_collide"):
        walk = [(n, r) for n, r in kernels.items() if stem in n]
        assert len(walk) == 2 and sum(stem + "_count" in n for n, _ in walk) == 1, "\n".join(kernels)
        for name, r in walk:
            assert int(r["Occupancy"]) >= 4 and int(r["ScratchSize"]) <= 32 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
    for stem, count in (("k_pairs_plan", 2), ("k_pairs_refs", 1)):
        ks = [(n, r) for n, r in kernels.items() if stem in n]
        assert len(ks) == count, "\n".join(kernels)
        for name, r in ks:
            assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)


def test_the_resource_report_names_every_earlier_kernel_unchanged():
    """profiles/instance_pairs.txt records the report of both libraries before and after the instance-pair kernels: every kernel of the
    earlier report is in the later one with the same figures"""
    text = open(os.path.join(ROOT, "profiles", "instance_pairs.txt")).read()
    for lib in ("product", "alt"):
        before = dict(re.findall(r"^before %s (\S+) (.*)$" % lib, text, re.M))
        after = dict(re.findall(r"^after %s (\S+) (.*)$" % lib, text, re.M))
        assert len(before) >= 70 and all(after.get(k) == v for k, v in before.items()), lib
        assert sum("k_pairs_" in k for k in after) == 8 and not any("k_pairs_" in k for k in before)


def test_the_tie_scene_has_a_tie():
    c = case("tie")
    rec = ipr.records(0, 1, 2.0)
    d2p = c.per_triangle_d2(rec[0])
    assert np.nanmin(d2p) == F(4.0) and (d2p == F(4.0)).sum() >= 2
    h, src, quv, _ = c.nearest(rec)
    assert h["t"][0] == F(2.0) and h["inst"][0] == 1 and src[0] == np.nonzero(d2p == F(4.0))[0][0]
    assert c.nearest(ipr.records(0, 1, np.nextafter(F(2.0), F(0))))[1][0] == -1      # (the bound is inclusive, and no wider)


def test_the_scenes_cross_the_boundaries():
    """the premises of the GPU tests, on the reference alone"""
    a, c = case("apart"), case("close")
    assert a.n_inst == 12 and sorted(set(a.count.tolist())) == [0, 8, 12, 80, 320] and a.count[BIG] == 320 and a.count[NOTHING] == 0
    recs = record_list(a.n_inst)
    assert len(recs) == 12 * 13
    ends = np.cumsum(a.count[recs[:, 0]])
    assert (ends[:-1] % 64 == 0).sum() >= 10 and (ends[:-1] % 64 != 0).sum() >= 100 and ends[-1] > 256 * 4
    assert (a.count[recs[:, 0]] > 64).any() and (a.count[recs[:, 0]] > 256).any()
    # apart: every admitted pair is apart; with the median radius some records hit and some miss
    h, src, _, _ = a.nearest(recs)
    hit = h["inst"] >= 0
    other = recs[:, 0] != recs[:, 1]
    assert hit.sum() > 60 and (h["t"][hit & other] > 0.05).all() and (h["t"][hit & ~other] == 0).all() and (src[hit] >= 0).all() and (src[~hit] == -1).all()
    assert not hit[recs[:, 0] == NOTHING].any() and not hit[recs[:, 0] == VOID].any() and not hit[recs[:, 1] == MASKED].any()
    assert hit[(recs[:, 0] == MASKED) & (recs[:, 1] == -1)].all() and hit[(recs[:, 0] == FLAT) & (recs[:, 1] == -1)].all()
    assert (src[hit] > 0).sum() > 40
    hm = a.nearest(with_radius(recs, median_radius(a, recs)))[0]
    assert 20 < (hm["inst"][hit] >= 0).sum() < hit.sum() - 20
    assert (a.overlaps(recs)[0][recs[:, 0] != recs[:, 1]] == 0).all()
    # close: bodies interpenetrate
    counts, first4 = c.overlaps(recs)
    print("close: %d of %d records without a contact, %d with more than 16 pairs, %d with a first p above 0, largest count %d" %
          ((counts == 0).sum(), len(recs), (counts > 16).sum(), (first4[:, 0] > 0).sum(), counts.max()))
    assert (counts == 0).sum() > 20 and (counts > 16).sum() > 10 and (first4[:, 0] > 0).sum() >= 1
    assert ((first4[:, 0] >= 0) == (counts > 0)).all()
    one = c.overlaps(recs, ONE_BIT)[0]
    assert 0 < (one > 0).sum() < (counts > 0).sum() and (c.overlaps(recs, 0)[0] == 0).all()
    # the invalid records are answered in the miss form
    bad = invalid_records(c)
    h, src, quv, _ = c.nearest(bad)
    assert (h["inst"] == -1).all() and (src == -1).all() and (quv == 0).all() and np.array_equal(h["t"].view(np.uint32), bad[:, 2].view(np.uint32))
    counts, first4 = c.overlaps(bad)
    no_radius = np.array([5, 6])      # (a negative or NaN radius: the overlap query ignores it, the record is valid)
    assert (np.delete(counts, no_radius) == 0).all() and (np.delete(first4, no_radius, axis=0) == [-1, -1, -1, 0]).all()
    assert counts[5] == counts[6] == c.overlaps(ipr.records(0, 1))[0][0]


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


def gpu_nearest(ctx, irefs, cull=0xFF):
    import torch
    res = ctx.closest_instances_device(dev(irefs), cull_mask=cull, attributes=True, params=True)
    torch.cuda.synchronize()
    h, a = res.numpy()
    return h, res.src_prim.cpu().numpy(), res.quv.cpu().numpy(), a


def gpu_overlap(ctx, irefs, cull=0xFF, **kw):
    import torch
    count, first4 = ctx.overlap_instances_device(dev(irefs), cull_mask=cull, **kw)
    torch.cuda.synchronize()
    return count.cpu().numpy().view(np.uint64), (first4.cpu().numpy() if first4 is not None else None)


def nearest_check(ctx, c, irefs, cull=0xFF, what=""):
    """twice the same bytes; hits, source primitives and (qu, qv) against the reference; hits, (qu, qv) and attributes against
    closest_scene_triangle_device on the same context for the winners' references"""
    import torch
    got = gpu_nearest(ctx, irefs, cull)
    again = gpu_nearest(ctx, irefs, cull)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), what + ": two runs differ"
    h, src, quv, a = got
    rh, rsrc, rquv, refs = c.nearest(irefs, cull)
    if src.tobytes() != rsrc.tobytes() or h.tobytes() != rh.tobytes():
        bad = np.nonzero((src != rsrc) | (h.view(np.uint8).reshape(len(h), -1) != rh.view(np.uint8).reshape(len(h), -1)).any(axis=1))[0]
        raise AssertionError("%s: %d records differ, first %d: record %s gpu %s p %d expected %s p %d" %
                             (what, len(bad), bad[0], irefs[bad[0]], h[bad[0]], src[bad[0]], rh[bad[0]], rsrc[bad[0]]))
    assert quv.tobytes() == rquv.tobytes(), what
    one = ctx.closest_scene_triangle_device(dev(refs), cull_mask=cull, attributes=True, params=True)
    torch.cuda.synchronize()
    oh, oa = one.numpy()
    assert h.tobytes() == oh.tobytes() and quv.tobytes() == one.quv.cpu().numpy().tobytes() and a.tobytes() == oa.tobytes(), what
    return rh, rsrc


def overlap_check(ctx, c, irefs, cull=0xFF, what=""):
    """twice the same bytes; counts and firsts against the reference; occupancy"""
    got = gpu_overlap(ctx, irefs, cull, first=True)
    again = gpu_overlap(ctx, irefs, cull, first=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again)), what + ": two runs differ"
    counts, first4 = c.overlaps(irefs, cull)
    assert got[0].tobytes() == counts.tobytes(), (what, np.nonzero(got[0] != counts)[0][:5])
    assert got[1].tobytes() == first4.tobytes(), (what, np.nonzero((got[1] != first4).any(axis=1))[0][:5])
    only, none = gpu_overlap(ctx, irefs, cull)
    assert none is None and only.tobytes() == counts.tobytes(), what
    occ, none = gpu_overlap(ctx, irefs, cull, any=True)
    assert none is None and np.array_equal(occ, (counts > 0).astype(np.uint64)), what + ", any"
    return counts, first4


def all_checks(ctx, c, what):
    recs = record_list(c.n_inst)
    nearest_check(ctx, c, recs, what=what)
    nearest_check(ctx, c, with_radius(recs, median_radius(c, recs)), what=what + ", median radius")
    overlap_check(ctx, c, recs, what=what)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["apart", "close"])
def test_distances(ctx, layout):
    """every ordered pair and every body against the others, with radii +inf, the median and 0, under cull masks 0xFF, one bit and 0"""
    c = case(layout)
    load(ctx, c.parts)
    recs = record_list(c.n_inst)
    rh, rsrc = nearest_check(ctx, c, recs, what=layout)
    assert (rh["inst"] >= 0).sum() > 60
    med = median_radius(c, recs)
    for r, cull in ((med, 0xFF), (0.0, 0xFF), (np.inf, ONE_BIT), (med, ONE_BIT), (np.inf, 0x00)):
        nearest_check(ctx, c, with_radius(recs, r), cull, what="%s, radius %g, cull %#x" % (layout, r, cull))


@pytest.mark.gpu
def test_distance_is_the_minimum_over_the_source_triangles(ctx):
    """t equals the minimum t of closest_scene_triangle_device over every source triangle of the record, on the same context"""
    import torch
    c = case("apart")
    load(ctx, c.parts)
    recs = record_list(c.n_inst)
    h, src, _, _ = gpu_nearest(ctx, recs)
    every, rec = ipr.every_triangle_of(c, recs)
    one = ctx.closest_scene_triangle_device(dev(every))
    torch.cuda.synchronize()
    oh, _ = one.numpy()
    for k in range(len(recs)):
        mine = oh[rec == k]
        hits = mine[mine["inst"] >= 0]
        if len(hits) == 0:
            assert h["inst"][k] == -1 and src[k] == -1
        else:
            assert h["t"][k] == hits["t"].min() and mine["t"][src[k]] == h["t"][k] and mine[src[k]].tobytes() == h[k].tobytes(), k


@pytest.mark.gpu
def test_ties_and_the_inclusive_radius(ctx):
    c = case("tie")
    load(ctx, c.parts)
    recs = ipr.records([0, 0, 1, 0, 1, 0], [1, -1, 0, 1, -1, 0], np.array([2.0, 2.0, 2.0, np.nextafter(F(2.0), F(0)), np.inf, np.inf], F))
    rh, rsrc = nearest_check(ctx, c, recs, what="tie scene")
    assert (rh["t"][[0, 1, 2, 4]] == F(2.0)).all() and rh["inst"][3] == -1 and rh["t"][5] == 0
    overlap_check(ctx, c, recs, what="tie scene")


@pytest.mark.gpu
def test_invalid_records_among_valid_ones(ctx):
    """they give the miss form and change no neighbour's answer"""
    c = case("close")
    load(ctx, c.parts)
    good = record_list(c.n_inst)[::7]
    bad = invalid_records(c)
    mixed = np.concatenate([bad[:4], good[:10], bad[4:], good[10:]])
    at = np.concatenate([np.arange(4, 14), np.arange(14 + len(bad) - 4, len(mixed))])
    h, src, quv, a = gpu_nearest(ctx, mixed)
    gh, gsrc, gquv, ga = gpu_nearest(ctx, good)
    assert h[at].tobytes() == gh.tobytes() and src[at].tobytes() == gsrc.tobytes() and quv[at].tobytes() == gquv.tobytes() and a[at].tobytes() == ga.tobytes()
    nearest_check(ctx, c, mixed, what="mixed")
    hb, sb, qb, ab = gpu_nearest(ctx, bad)
    assert (hb["inst"] == -1).all() and (hb["prim"] == -1).all() and (sb == -1).all() and (qb == 0).all()
    assert np.array_equal(hb["t"].view(np.uint32), bad[:, 2].view(np.uint32)) and (hb["u"] == 0).all() and (hb["v"] == 0).all()
    assert (ab[:, [0, 1, 2, 4, 5, 6, 7]] == 0).all() and (ab[:, 3] == -1).all()
    overlap_check(ctx, c, mixed, what="mixed")
    counts, first4 = gpu_overlap(ctx, mixed, first=True)
    gc, gf = gpu_overlap(ctx, good, first=True)
    assert counts[at].tobytes() == gc.tobytes() and first4[at].tobytes() == gf.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["apart", "close"])
def test_overlaps(ctx, layout):
    import torch
    c = case(layout)
    load(ctx, c.parts)
    recs = record_list(c.n_inst)
    counts, first4 = overlap_check(ctx, c, recs, what=layout)
    for cull in (ONE_BIT, 0x00):
        overlap_check(ctx, c, recs, cull, what="%s, cull %#x" % (layout, cull))
    # the sum of the per-triangle counts of the same context
    every, rec = ipr.every_triangle_of(c, recs)
    one = ctx.overlap_scene_triangles_device(dev(every), max_ids=1)
    torch.cuda.synchronize()
    oc, oi = one.numpy()
    sums = np.zeros(len(recs), np.uint64)
    np.add.at(sums, rec, oc.astype(np.uint64))
    assert sums.tobytes() == counts.tobytes()
    if layout == "close":
        assert (counts > 16).sum() > 10
        for k in np.nonzero(counts > 0)[0][:40]:
            rows = np.nonzero(rec == k)[0]
            p = np.nonzero(oc[rows] > 0)[0][0]
            assert first4[k].tolist() == [p, oi[rows[p], 0, 0], oi[rows[p], 0, 1], 0]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["rt_set_instances", "rt_set_instances_device"])
def test_tlas_producers_and_an_update(device):
    a, c = case("apart"), case("close")
    ctx = RtContext(0)
    try:
        load(ctx, a.parts, device)
        all_checks(ctx, a, "built")
        load(ctx, c.parts, device, update=True)
        all_checks(ctx, c, "updated")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "1", "2"])
def test_blas_builders_and_a_refit(builder, monkeypatch):
    """the same bytes whatever builder made the trees, and after rt_refit_blas_device with moved vertices and a TLAS update those of the
    reference over the new vertices"""
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
            p[:, :3] *= (1.0 + 0.2 * np.sin(5.0 * p[:, [1, 2, 0]])).astype(F)
            torch.cuda.synchronize()
            ctx.refit_blas_device(mesh, dev(p))
        torch.cuda.synchronize()
        ctx.set_instances_device(dev_inst(inst), update=True)
        if "refit" not in _CASES:
            _CASES["refit"] = ipr.Pairs((v2, idx, ranges, inst))
        new = case("refit")
        assert new.sc.a.tobytes() != c.sc.a.tobytes()
        all_checks(ctx, new, "refit, builder " + builder)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_host_forms_and_counting(ctx):
    c = case("close")
    load(ctx, c.parts)
    recs = record_list(c.n_inst)
    h, src, quv, _ = gpu_nearest(ctx, recs)
    hh, hsrc, hquv, st = ctx.closest_instances(recs, params=True)
    assert hh.tobytes() == h.tobytes() and hsrc.tobytes() == src.tobytes() and hquv.tobytes() == quv.tobytes()
    assert st.node_visits == 0 and st.tri_tests == 0 and st.ms_trace_closest > 0 and st.bvh_node_bytes == 32
    hh, hsrc, st = ctx.closest_instances(recs.view(api.INST_REF_DTYPE).reshape(-1), counting=True)
    assert hh.tobytes() == h.tobytes() and hsrc.tobytes() == src.tobytes() and st.node_visits > 0 and st.tri_tests > 0
    counts, first4 = gpu_overlap(ctx, recs, first=True)
    hc, hf, st = ctx.overlap_instances(recs, first=True)
    assert hc.tobytes() == counts.tobytes() and hf.tobytes() == first4.tobytes() and st.node_visits == 0 and st.ms_trace_closest > 0
    hc, hf, st = ctx.overlap_instances(recs, counting=True)
    assert hc.tobytes() == counts.tobytes() and hf is None and st.node_visits > 0 and st.tri_tests >= int(counts.sum())
    hc, hf, st_any = ctx.overlap_instances(recs, any=True, counting=True)
    assert np.array_equal(hc, (counts > 0).astype(np.uint64)) and 0 < st_any.node_visits
    # out= reuse
    import torch
    d = dev(recs)
    res = ctx.closest_instances_device(d, attributes=True, params=True)
    res2 = ctx.closest_instances_device(d, attributes=True, params=True, out=(res.hits, res.attr, res.src_prim, res.quv))
    torch.cuda.synchronize()
    assert res2.hits is res.hits and res2.src_prim is res.src_prim and res.numpy()[0].tobytes() == h.tobytes()
    cnt = torch.empty((len(recs),), dtype=torch.int64, device="cuda:0")
    c2, f2 = ctx.overlap_instances_device(d, out=(cnt, None))
    torch.cuda.synchronize()
    assert c2 is cnt and f2 is None and cnt.cpu().numpy().view(np.uint64).tobytes() == counts.tobytes()


@pytest.mark.gpu
def test_error_returns_and_an_empty_call():
    import torch
    c = case("tie")
    ctx = RtContext(0)
    try:
        L, h = ctx.L, ctx.h
        vp = ctypes.c_void_p
        n = 4
        recs = dev(ipr.records([0, 1, 0, 1], [1, 0, -1, -1]))
        hits = torch.zeros((n + 1, 5), dtype=torch.int32, device="cuda:0")
        src = torch.zeros((n + 1,), dtype=torch.int32, device="cuda:0")
        cnt = torch.zeros((n + 1,), dtype=torch.int64, device="cuda:0")
        f4 = torch.zeros((n + 1, 4), dtype=torch.int32, device="cuda:0")
        R, H, S, C64, F4 = recs.data_ptr(), hits.data_ptr(), src.data_ptr(), cnt.data_ptr(), f4.data_ptr()
        p = lambda x: vp(x) if x else None   # noqa: E731
        near = lambda n_, r, hh, ss, mask=0xFF: L.rt_closest_instances_device(h, n_, p(r), mask, p(hh), p(ss), None, None, None)   # noqa: E731
        over = lambda n_, r, cc, ff, flags=0, mask=0xFF: L.rt_overlap_instances_device(h, n_, p(r), mask, flags, p(cc), p(ff), None)   # noqa: E731
        # before the geometry and the instances are set
        assert near(n, R, H, S) == RT_ERR_NOT_READY and over(n, R, C64, 0) == RT_ERR_NOT_READY
        verts, idx, ranges, inst = c.parts
        ctx.upload_geometry(verts, idx, ranges)
        assert near(n, R, H, S) == RT_ERR_NOT_READY and over(n, R, C64, 0) == RT_ERR_NOT_READY
        ctx.set_instances(inst)
        assert near(n, R, H, S) == 0 and over(n, R, C64, F4) == 0
        torch.cuda.synchronize()
        want = c.nearest(recs.cpu().numpy())
        assert hits.cpu().numpy()[:n].tobytes() == want[0].view(np.int32).tobytes() and src.cpu().numpy()[:n].tobytes() == want[1].tobytes()
        # NULL and misaligned pointers
        for args in ((0, H, S), (R, 0, S), (R, H, 0), (R + 4, H, S), (R, H + 2, S), (R, H, S + 1)):
            assert near(n, *args) == RT_ERR_INVALID_ARGUMENT, args
        for args in ((0, C64, 0), (R, 0, 0), (R + 8, C64, 0), (R, C64 + 4, 0), (R, C64, F4 + 2)):
            assert over(n, *args) == RT_ERR_INVALID_ARGUMENT, args
        assert L.rt_closest_instances_device(h, n, vp(R), 0xFF, vp(H), vp(S), vp(H + 4), None, None) == RT_ERR_INVALID_ARGUMENT    # attributes: 16 bytes
        assert L.rt_closest_instances_device(h, n, vp(R), 0xFF, vp(H), vp(S), None, vp(H + 2), None) == RT_ERR_INVALID_ARGUMENT    # parameters: 4 bytes
        host_mem = np.zeros(64, np.int32)
        assert near(n, host_mem.ctypes.data, H, S) == RT_ERR_INVALID_ARGUMENT
        # d_first4 with RT_OVERLAP_ANY, unknown flag bits, the cull mask
        assert over(n, R, C64, F4, flags=api.OVERLAP_ANY) == RT_ERR_INVALID_ARGUMENT and over(n, R, C64, 0, flags=api.OVERLAP_ANY) == 0
        assert over(n, R, C64, 0, flags=2) == RT_ERR_INVALID_ARGUMENT and over(n, R, C64, 0, flags=0x80000001) == RT_ERR_INVALID_ARGUMENT
        assert over(n, R, C64, 0, mask=0x100) == RT_ERR_INVALID_ARGUMENT and near(n, R, H, S, mask=0x100) == RT_ERR_INVALID_ARGUMENT
        # the conservative size check: n x 12 triangles
        big = (0xFFFFFF00 + 11) // 12
        assert near(big, R, H, S) == RT_ERR_INVALID_ARGUMENT and over(big, R, C64, 0) == RT_ERR_INVALID_ARGUMENT
        assert near(0xFFFFFF00, R, H, S) == RT_ERR_INVALID_ARGUMENT
        st = api.RtStats()
        out = np.zeros(1, HIT_DTYPE)
        assert L.rt_closest_instances(h, big, vp(host_mem.ctypes.data), 0xFF, vp(out.ctypes.data), vp(host_mem.ctypes.data), None, 0, ctypes.byref(st)) == RT_ERR_INVALID_ARGUMENT
        assert L.rt_overlap_instances(h, n, vp(host_mem.ctypes.data), 0xFF, 0, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
        with pytest.raises(RtError):
            ctx.closest_instances(ipr.records([0], [1]), cull_mask=0x100)
        with pytest.raises(ValueError):
            ctx.overlap_instances_device(recs, any=True, first=True)
        # n == 0: nothing is enqueued, nothing is written
        torch.cuda.synchronize()
        hits.fill_(77); src.fill_(77); cnt.fill_(77)
        assert near(0, R, H, S) == 0 and near(0, 0, 0, 0) == 0 and over(0, R, C64, 0) == 0 and over(0, 0, 0, 0) == 0
        torch.cuda.synchronize()
        assert (hits == 77).all() and (src == 77).all() and (cnt == 77).all()
        empty = ctx.closest_instances_device(dev(np.zeros((0, 4), np.int32)))
        assert tuple(empty.hits.shape) == (0, 5) and tuple(empty.src_prim.shape) == (0,)
        assert ctx.closest_instances(np.zeros((0, 4), np.int32))[0].shape == (0,) and ctx.overlap_instances(np.zeros((0, 4), np.int32))[0].shape == (0,)
        # the rows beyond n were never touched by the calls above
        assert (f4[n:] == 0).all()
    finally:
        ctx.close()
