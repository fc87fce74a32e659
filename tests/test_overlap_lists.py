"""rt_overlap_boxes_device_list, rt_overlap_triangles_device_list, rt_overlap_scene_triangles_device_list and their host forms
(include/rt_api.h "Overlap lists"; DESIGN.md §5 "Overlap lists"): the whole candidate set of every record in CSR form.

The candidate sets are the capped calls', so the references are theirs (tests/overlap_list_reference.py puts them into CSR form) and the
GPU is held to them byte for byte: offsets, ids, the rows a capacity lets through and every byte it does not.  The scenes, the record
sets and their brute-force pairs are those of tests/test_overlap_boxes.py, tests/test_triangle_overlaps.py and
tests/test_scene_triangles.py, imported and computed once."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import closest_reference as cr
from tests import overlap_list_reference as olr
from tests import scene_triangle_reference as stf
from tests import test_overlap_boxes as tob
from tests import test_scene_triangles as tst
from tests import test_triangle_overlaps as tto
from tests.test_ray_query import dev_inst, slow_queue
from tests.test_ray_query_oracle import use_builder
from vulkan_raytracing_amd import RtContext, api
from vulkan_raytracing_amd.api import RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
NAMES = ("boxes", "triangles", "scene_triangles")
CULLS = (0xFF, 0x01, 0x5A, 0x00)

_CSR = {}


def _pairs(kind, name, key):
    """the pairs of set `key` of scene `name` under cull mask 0xFF and which of them are candidates, computed once: a narrower mask
    admits a subset of the instances and changes no pair that stays"""
    k = (kind, name, key)
    if k not in _CSR:
        mod, ref = (tob, tob.orf) if kind == "b" else (tto, tto.trf)
        parts, sc, tris, sets, _ = mod.scene_and_sets(name)
        bi, ti = ref.surviving_pairs(tris, sets[key], 0xFF)
        _CSR[k] = (sc, len(sets[key]), bi, ti, ref.candidates32(tris, sets[key], bi, ti))
    return _CSR[k]


def box_csr(name, key, cull=0xFF, kind="b"):
    """the CSR reference of box set `key` of scene `name` under `cull`, computed once"""
    k = (kind, name, key, cull)
    if k not in _CSR:
        sc, n, bi, ti, keep = _pairs(kind, name, key)
        _CSR[k] = olr.csr(sc, n, bi, ti, keep & sc.admitted(cull)[ti])
    return _CSR[k]


def tri_csr(name, key, cull=0xFF):
    return box_csr(name, key, cull, kind="t")


def ref_sets():
    """the references of the scene of tests/test_scene_triangles.py: every triangle against every other instance, and every triangle
    of the first eight instances against each of them"""
    c = tst.case("close")
    return c, {"others": stf.every_triangle(c.sc, -1), "pairs": tst.pair_refs(c)}


def refs_csr(key, cull=0xFF):
    k = ("r", key, cull)
    if k not in _CSR:
        c, sets = ref_sets()
        _CSR[k] = olr.refs_csr(c.src, sets[key], cull)
    return _CSR[k]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def test_exports_abi_and_null_context():
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    L = api.lib()
    assert L.rt_abi_version() == 7
    rec = {"boxes": r"const void\* d_boxes8", "triangles": r"const void\* d_tris12", "scene_triangles": r"const void\* d_refs4"}
    host = {"boxes": r"const float\* boxes8_host", "triangles": r"const float\* tris12_host", "scene_triangles": r"const rt_tri_ref\* refs_host"}
    for name in NAMES:
        d, h = "rt_overlap_%s_device_list" % name, "rt_overlap_%s_list" % name
        assert d in api.EXPORTS and h in api.EXPORTS
        assert re.search(r"^int %s\(rt_ctx\* ctx, size_t n, %s, uint32_t cull_mask, uint32_t flags,\s+void\* d_offsets, void\* d_ids, size_t capacity, "
                         r"void\* hip_stream\);" % (d, rec[name]), hdr, re.M), d
        assert re.search(r"^int %s\(rt_ctx\* ctx, size_t n, %s, uint32_t cull_mask, uint32_t flags,\s+uint64_t\* offsets_host, int32_t\* ids_host, "
                         r"size_t capacity, int counting, rt_stats\* stats\);" % (h, host[name]), hdr, re.M), h
        assert hasattr(L, d) and hasattr(L, h)
        assert getattr(L, d)(None, 0, None, 0xFF, 0, None, None, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert getattr(L, d)(None, 64, None, 0xFF, 0, None, None, 64, None) == RT_ERR_INVALID_ARGUMENT
        assert getattr(L, h)(None, 0, None, 0xFF, 0, None, None, 0, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert hasattr(RtContext, "overlap_%s_device_list" % name) and hasattr(RtContext, "overlap_%s_list" % name)
    assert hasattr(api, "OverlapList")
    ins, tile = olr.thresholds()
    assert 1 <= ins < tile and tile & (tile - 1) == 0


@pytest.mark.parametrize("name", ["small", "soup", "lattice"])
def test_csr_against_the_capped_references(name):
    """csr(...) holds exactly what rows(..., max_ids=16) and the counts hold: the first min(count, 16) entries of every row and
    diff(offsets), on every set of the three scenes, for boxes and for query triangles"""
    for scene_and_sets, fn in ((tob.scene_and_sets, box_csr), (tto.scene_and_sets, tri_csr)):
        parts, sc, tris, sets, ref = scene_and_sets(name)
        for key in sets:
            offsets, ids = fn(name, key)
            rc, ri = ref[key]
            assert offsets.dtype == np.uint64 and ids.dtype == np.int32 and ids.shape == (int(offsets[-1]), 2)
            assert np.array_equal(np.diff(offsets.astype(np.int64)), rc.astype(np.int64)), (name, key)
            pc, pr = olr.prefix_rows(offsets, ids)
            assert pc.tobytes() == rc.tobytes() and pr.tobytes() == ri.tobytes(), (name, key)
            for i in np.nonzero(rc > 1)[0][:50]:   # every row ascending by (inst, prim), strictly
                row = ids[int(offsets[i]):int(offsets[i + 1])].astype(np.int64)
                key64 = row[:, 0] * (1 << 32) + row[:, 1]
                assert (np.diff(key64) > 0).all()
    if name == "small":
        c, sets = ref_sets()
        for key, r in sets.items():
            offsets, ids = refs_csr(key)
            rc, ri = c.overlaps(r)
            pc, pr = olr.prefix_rows(offsets, ids)
            assert pc.tobytes() == rc.tobytes() and pr.tobytes() == ri.tobytes(), key


def test_the_written_rows_rule():
    """the rule restated on hand-made offsets: capacity 0, inside a row, exactly at a row's end, at T and above T"""
    offsets = np.array([0, 3, 3, 7, 7, 12], np.uint64)   # rows of 3, 0, 4, 0, 5
    ids = np.arange(24, dtype=np.int32).reshape(12, 2)
    F = olr.FILL
    assert not olr.written(offsets, 0)[[0, 2, 4]].any() and len(olr.expected_ids(offsets, ids, 0)) == 0
    assert olr.written(offsets, 5).tolist() == [True, True, False, False, False]
    e = olr.expected_ids(offsets, ids, 5)
    assert e[:24].tobytes() == ids[:3].tobytes() and (e[24:] == F).all() and len(e) == 40
    assert olr.written(offsets, 7).tolist() == [True, True, True, True, False]
    e = olr.expected_ids(offsets, ids, 7)
    assert e.tobytes() == ids[:7].tobytes()
    e = olr.expected_ids(offsets, ids, 11)   # one short of T: the last row is not written at all
    assert e[:56].tobytes() == ids[:7].tobytes() and (e[56:] == F).all()
    assert olr.written(offsets, 12).all() and olr.expected_ids(offsets, ids, 12).tobytes() == ids.tobytes()
    e = olr.expected_ids(offsets, ids, 20)
    assert e[:96].tobytes() == ids.tobytes() and (e[96:] == F).all() and len(e) == 160


def strip_case():
    """the strip, its rows of every length around the two thresholds and above the tile, long rows between empty and short ones, and
    their CSR reference; the premise (every length is reached) is asserted here, on the CPU"""
    if "strip" not in _CSR:
        ins, tile = olr.thresholds()
        lens = sorted({0, 1, ins - 1, ins, ins + 1, tile - 1, tile, tile + 1, 2 * tile + 3})
        parts = olr.strip_scene(2 * tile + 8)
        sc = cr.Scene(*parts)
        rows, want = [], []
        for m in lens:
            rows += [olr.strip_box(0), olr.strip_box(m), olr.strip_box(3)]
            want += [0, m, 3]
        rows += [olr.strip_box(100, both=True), olr.strip_box(tile // 2 + 1, both=True), olr.strip_box(0)]
        want += [200, tile + 2, 0]
        boxes = np.stack(rows)
        offsets, ids = olr.boxes_csr(sc, boxes)
        assert np.diff(offsets.astype(np.int64)).tolist() == want
        _CSR["strip"] = (parts, boxes, offsets, ids, lens)
    return _CSR["strip"]


def test_the_strip_reaches_every_length():
    parts, boxes, offsets, ids, lens = strip_case()
    ins, tile = olr.thresholds()
    got = set(np.diff(offsets.astype(np.int64)).tolist())
    assert {0, 1, ins - 1, ins, ins + 1, tile - 1, tile, tile + 1} <= got and max(got) > 2 * tile
    long_row = ids[int(offsets[-4]):int(offsets[-3])]   # both instances in one row
    assert set(long_row[:, 0].tolist()) == {0, 1}


@pytest.mark.parametrize("target", ["resource-usage", "resource-usage-alt"])
def test_list_kernels_keep_their_budget(target):
    """six new walk kernels (boxes, triangles, references; each with its counting form) within the record-level walks' budget (>= 4 waves
    per SIMD, scratch <= 32 bytes, no spills, the 12 KB stack in LDS); the sort kernel without scratch or spills, its LDS the tile"""
    from tests.test_ray_query import _resource_usage
    kernels = _resource_usage(target)
    new = {n: r for n, r in kernels.items() if "k_list_" in n}
    walk = {n: r for n, r in new.items() if re.search(r"k_list_(boxes|triangles|refs)(_count)?E", n)}
    assert len(walk) == 6 and sum("_count" in n for n in walk) == 3, "\n".join(new)
    for name, r in walk.items():
        assert int(r["Occupancy"]) >= 4 and int(r["ScratchSize"]) <= 32 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert int(r["LDS Size"]) == 12288, (name, r)
    sort = [r for n, r in new.items() if "k_list_sort" in n]
    assert len(sort) == 1
    assert int(sort[0]["ScratchSize"]) == 0 and int(sort[0]["VGPRs Spill"]) == 0 and int(sort[0]["SGPRs Spill"]) == 0
    assert int(sort[0]["LDS Size"]) == 8 * olr.thresholds()[1]
    for n, r in new.items():
        if "k_list_scan" in n:
            assert int(r["ScratchSize"]) == 0 and int(r["VGPRs Spill"]) == 0, (n, r)
    assert len(new) == 10, "\n".join(new)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


def dev(kind, records):
    import torch
    if kind == "scene_triangles":
        return torch.from_numpy(np.ascontiguousarray(records, np.int32).reshape(-1, 4)).to("cuda:0")
    return torch.from_numpy(np.ascontiguousarray(records, np.float32).reshape(-1, 8 if kind == "boxes" else 12)).to("cuda:0")


def gpu_list(c, kind, records, capacity, cull=0xFF, **kw):
    """(offsets uint64 (n + 1,), ids int32 (capacity, 2) or None) of the device call"""
    import torch
    res = getattr(c, "overlap_%s_device_list" % kind)(dev(kind, records), capacity=capacity, cull_mask=cull, **kw)
    torch.cuda.synchronize()
    return res.numpy()


def gpu_capped(c, kind, records, cull=0xFF):
    import torch
    res = getattr(c, "overlap_%s_device" % kind)(dev(kind, records), max_ids=16, cull_mask=cull)
    torch.cuda.synchronize()
    return res.numpy()


def check(got, ref, what):
    """(offsets, ids) of the GPU against the reference's, byte for byte"""
    offsets, ids = got
    ro, ri = ref
    if offsets.tobytes() != ro.tobytes():
        bad = np.nonzero(offsets != ro)[0]
        raise AssertionError("%s: %d offsets differ, first at %d: gpu %d reference %d" % (what, len(bad), bad[0], offsets[bad[0]], ro[bad[0]]))
    if len(ri) == 0:
        assert ids is None or len(ids) == 0, what
        return
    if ids.tobytes() != ri.tobytes():
        bad = np.nonzero((ids != ri).any(axis=1))[0]
        row = int(np.searchsorted(ro, bad[0], side="right")) - 1
        raise AssertionError("%s: %d entries differ, first at %d (row %d of length %d): gpu %s reference %s"
                             % (what, len(bad), bad[0], row, int(ro[row + 1] - ro[row]), ids[bad[0]].tolist(), ri[bad[0]].tolist()))


def check_all(c, kind, records, ref, what, cull=0xFF):
    """the list call with capacity == T against the reference, and the capped call's rows and counts against the lists' prefixes"""
    got = gpu_list(c, kind, records, int(ref[0][-1]), cull)
    check(got, ref, what)
    counts, rows = gpu_capped(c, kind, records, cull)
    pc, pr = olr.prefix_rows(got[0], got[1] if got[1] is not None else np.zeros((0, 2), np.int32))
    assert counts.tobytes() == pc.tobytes() and rows.tobytes() == pr.tobytes(), what + ": the capped call"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "teapot", "soup", "sliver"])
def test_every_box_set(ctx, name):
    """every box set byte for byte with capacity == T, the enclosing box of `mixed` (the long row; through the spill half of the stack)
    among them, under four cull masks; the capped call's rows are the prefixes"""
    parts, sc, tris, sets, ref = tob.scene_and_sets(name)
    tob.load(ctx, parts)
    for key, boxes in sets.items():
        check_all(ctx, "boxes", boxes, box_csr(name, key), "%s %s" % (name, key))
    longest = int(np.diff(box_csr(name, "mixed")[0].astype(np.int64)).max())
    assert longest == sc.admitted(0xFF).sum()
    if name in ("small", "teapot"):   # (the sliver scene and the soup hold 168 and 144 triangles)
        assert longest > olr.thresholds()[1] or name == "small"
    for cull in CULLS[1:]:
        check_all(ctx, "boxes", sets["mixed"], box_csr(name, "mixed", cull), "%s mixed cull %#x" % (name, cull), cull)


@pytest.mark.gpu
def test_voxels_on_the_integer_lattice(ctx):
    parts, sc, tris, sets, ref = tob.scene_and_sets("lattice")
    tob.load(ctx, parts)
    check_all(ctx, "boxes", sets["voxels"], box_csr("lattice", "voxels"), "lattice voxels")
    assert (np.diff(box_csr("lattice", "voxels")[0].astype(np.int64)) == 0).sum() > 1000   # (most voxels touch nothing)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "teapot", "soup", "sliver", "lattice"])
def test_every_query_triangle_set(ctx, name):
    parts, sc, tris, sets, ref = tto.scene_and_sets(name)
    tto.load(ctx, parts)
    for key, q in sets.items():
        check_all(ctx, "triangles", q, tri_csr(name, key), "%s %s" % (name, key))
    if name != "lattice":
        for cull in CULLS[1:]:
            check_all(ctx, "triangles", sets["mixed"], tri_csr(name, "mixed", cull), "%s mixed cull %#x" % (name, cull), cull)


@pytest.mark.gpu
def test_references_against_the_others_and_against_one(ctx):
    """against = -1 and against = b on the interpenetrating scene of tests/test_scene_triangles.py"""
    c, sets = ref_sets()
    tst.load(ctx, c.parts)
    for key, r in sets.items():
        for cull in CULLS:
            check_all(ctx, "scene_triangles", r, refs_csr(key, cull), "references %s cull %#x" % (key, cull), cull)


@pytest.mark.gpu
def test_row_lengths_at_every_threshold(ctx):
    """rows of 0, 1, T - 1, T, T + 1 entries for the insertion threshold and the LDS tile, rows above the tile and across two
    instances, long rows between empty and short ones: stored shuffled, so the walk meets no row in order"""
    parts, boxes, offsets, ids, lens = strip_case()
    tob.load(ctx, parts)
    check_all(ctx, "boxes", boxes, (offsets, ids), "strip")


@pytest.mark.gpu
def test_capacity(ctx):
    """capacity 0 / NULL, T - 1, inside a middle row, exactly a row's end, T and T + 1000 on an ids buffer filled with 0x7F bytes: the
    written rows are exactly those of the rule, every other byte stays 0x7F, the offsets are complete every time"""
    import torch
    parts, sc, tris, sets, ref = tob.scene_and_sets("small")
    tob.load(ctx, parts)
    offsets, ids = box_csr("small", "mixed")
    off = offsets.astype(np.int64)
    T = int(off[-1])
    length = np.diff(off)
    mid = [i for i in np.nonzero(length >= 3)[0] if T // 3 < off[i] < 2 * T // 3]
    ins = olr.thresholds()[0]
    assert mid and (length > ins).sum() >= 10 and ((length > 0) & (length <= ins)).sum() >= 10   # rows of both kinds take part
    i = int(mid[len(mid) // 2])
    src = dev("boxes", sets["mixed"])
    for cap in (0, T - 1, int(off[i]) + 1, int(off[i + 1]), T, T + 1000):
        o_t = torch.full((len(off),), -1, dtype=torch.int64, device="cuda:0")
        i_t = torch.full((cap, 2), 0x7F7F7F7F, dtype=torch.int32, device="cuda:0") if cap else None
        res = ctx.overlap_boxes_device_list(src, out=(o_t, i_t))
        torch.cuda.synchronize()
        assert res.offsets.data_ptr() == o_t.data_ptr() and int(res.total) == T
        assert o_t.cpu().numpy().view(np.uint64).tobytes() == offsets.tobytes(), cap
        if cap == 0:
            assert res.ids is None
            continue
        got = i_t.cpu().numpy().view(np.uint8).reshape(-1)
        want = olr.expected_ids(offsets, ids, cap)
        if got.tobytes() != want.tobytes():
            bad = np.nonzero(got != want)[0]
            raise AssertionError("capacity %d: %d bytes differ, first in record %d" % (cap, len(bad), bad[0] // 8))
    # the reference triangles and the query triangles share the rule: one capacity inside a row each
    c, rsets = ref_sets()
    for kind, records, (ro, ri), loader, p in (("triangles", tto.scene_and_sets("small")[3]["mixed"], tri_csr("small", "mixed"), tto.load, tto.scene_and_sets("small")[0]),
                                               ("scene_triangles", rsets["others"], refs_csr("others"), tst.load, c.parts)):
        loader(ctx, p)
        cap = int(ro[-1]) // 2 + 1
        i_t = torch.full((cap, 2), 0x7F7F7F7F, dtype=torch.int32, device="cuda:0")
        o_t = torch.empty((len(ro),), dtype=torch.int64, device="cuda:0")
        getattr(ctx, "overlap_%s_device_list" % kind)(dev(kind, records), out=(o_t, i_t))
        torch.cuda.synchronize()
        assert o_t.cpu().numpy().view(np.uint64).tobytes() == ro.tobytes(), kind
        assert i_t.cpu().numpy().view(np.uint8).reshape(-1).tobytes() == olr.expected_ids(ro, ri, cap).tobytes(), kind


def tree_inputs():
    """boxes (the enclosing one among them), query triangles and references of the small scene, with their references before and after
    every instance moves"""
    if "tree" not in _CSR:
        parts, sc0, tris0, bsets, _ = tob.scene_and_sets("small")
        tsets = tto.scene_and_sets("small")[3]
        verts, idx, ranges, inst = parts
        rng = np.random.default_rng(72)
        moved = inst.copy()
        moved["transform"][:, [3, 7, 11]] += rng.uniform(-0.3, 0.3, (len(inst), 3)).astype(np.float32)
        lo, hi = tob.scene_box(sc0)
        boxes = np.concatenate([bsets["mixed"][:700], bsets["surface"][:300], tob.as_boxes(lo[None] - 2, hi[None] + 2), bsets["features"][:300]])
        q = np.concatenate([tsets["mixed"][:600], tsets["features"][:300]])
        r = np.concatenate([stf.every_triangle(sc0, -1), stf.refs(sc0.inst[:100], sc0.prim[:100], 3)])
        out = {"parts": parts, "moved_inst": moved, "records": {"boxes": boxes, "triangles": q, "scene_triangles": r}}
        for tag, records in (("first", inst), ("moved", moved)):
            sc = cr.Scene(verts, idx, ranges, records)
            src = stf.Source(sc, verts, idx, ranges, records)
            out[tag] = {"boxes": olr.boxes_csr(sc, boxes), "triangles": olr.triangles_csr(sc, q), "scene_triangles": olr.refs_csr(src, r)}
        _CSR["tree"] = out
    return _CSR["tree"]


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "unset", "1", "2"])
def test_whatever_the_tree(builder, monkeypatch):
    """the host builder and RT_GPU_BVH_ALGO unset / 1 / 2, host and device instance records with their TLAS updates: every result equals
    one reference, so the bytes are identical across trees although every tree is walked in an order of its own"""
    import torch
    t = tree_inputs()
    verts, idx, ranges, inst = t["parts"]
    c = RtContext(0)
    try:
        if builder == "unset":
            monkeypatch.delenv("RT_GPU_BVH_ALGO", raising=False)
            c.set_param("blas_builder", 1)
        else:
            use_builder(c, builder, monkeypatch)
        c.upload_geometry(verts, idx, ranges)
        for source in ("host", "device"):
            for records, update, tag in ((inst, False, "first"), (t["moved_inst"], True, "moved")):
                if source == "host":
                    c.set_instances(records, update=update)
                else:
                    torch.cuda.synchronize()
                    c.set_instances_device(dev_inst(records), update=update)
                for kind in NAMES:
                    ref = t[tag][kind]
                    check(gpu_list(c, kind, t["records"][kind], int(ref[0][-1])), ref, "%s, %s records, update %d, builder %s" % (kind, source, update, builder))
        assert np.diff(t["first"]["boxes"][0].astype(np.int64)).max() > olr.thresholds()[0]   # (the enclosing box: a row k_list_sort orders)
    finally:
        c.close()


@pytest.mark.gpu
def test_after_a_blas_refit():
    """a deformed mesh refitted on the GPU: not ready until the instances are set again, then the fresh build's bytes and the reference's"""
    import torch
    from tests.test_blas_refit import deform, with_mesh
    t = tree_inputs()
    verts, idx, ranges, inst = t["parts"]
    geom = types.SimpleNamespace(verts=verts, idx=idx, ranges=ranges)
    boxes = t["records"]["boxes"]
    c, fresh = RtContext(0), RtContext(0)
    try:
        tob.load(c, t["parts"])
        d = deform(geom, 0, amp=0.2)
        torch.cuda.synchronize()
        c.refit_blas_device(0, d)
        torch.cuda.synchronize()
        src = dev("boxes", boxes)
        o_t = torch.empty((len(boxes) + 1,), dtype=torch.int64, device="cuda:0")
        rc = c.L.rt_overlap_boxes_device_list(c.h, len(boxes), ctypes.c_void_p(src.data_ptr()), 0xFF, 0, ctypes.c_void_p(o_t.data_ptr()), None, 0, None)
        assert rc == RT_ERR_NOT_READY
        c.set_instances_device(dev_inst(inst))
        v2 = with_mesh(geom, verts, 0, d)
        tob.load(fresh, (v2, idx, ranges, inst))
        ref = olr.boxes_csr(cr.Scene(v2, idx, ranges, inst), boxes)
        got, want = gpu_list(c, "boxes", boxes, int(ref[0][-1])), gpu_list(fresh, "boxes", boxes, int(ref[0][-1]))
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        check(got, ref, "after the refit")
    finally:
        c.close()
        fresh.close()


@pytest.mark.gpu
def test_plumbing(ctx):
    """a caller's stream with the records made by a kernel queued just before the call; out= reuse; capacity=None (the exact
    allocation); n == 0; host forms equal device forms and counting fills the counters of both walks"""
    import torch
    parts, sc, tris, sets, ref = tob.scene_and_sets("small")
    tob.load(ctx, parts)
    boxes = sets["mixed"]
    r = box_csr("small", "mixed")
    T = int(r[0][-1])
    src = dev("boxes", boxes)
    # capacity=None: offsets first, the total read on the host, then exactly T records
    res = ctx.overlap_boxes_device_list(src)
    torch.cuda.synchronize()
    assert res.ids.shape == (T, 2) and res.offsets.dtype == torch.int64 and res.total.dim() == 0 and int(res.total) == T
    check(res.numpy(), r, "capacity=None")
    # out= reuse with room to spare: only the first T records are written
    o_t = torch.empty((len(boxes) + 1,), dtype=torch.int64, device="cuda:0")
    i_t = torch.full((T + 64, 2), 0x7F7F7F7F, dtype=torch.int32, device="cuda:0")
    res = ctx.overlap_boxes_device_list(src, out=(o_t, i_t))
    torch.cuda.synchronize()
    assert res.ids.data_ptr() == i_t.data_ptr() and res.offsets.data_ptr() == o_t.data_ptr()
    assert i_t.cpu().numpy().view(np.uint8).reshape(-1).tobytes() == olr.expected_ids(r[0], r[1], T + 64).tobytes()
    with pytest.raises(ValueError):
        ctx.overlap_boxes_device_list(src, out=(o_t[:-1], i_t))
    with pytest.raises(ValueError):
        ctx.overlap_boxes_device_list(src, capacity=5, out=(o_t, i_t))
    # stream order: the boxes are made by a kernel behind a slow queue on a side stream, and overwritten right after the call
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        a = slow_queue(torch, 12)
        p = (src + (a[0, 0] != a[0, 0]).to(torch.float32) * 0).contiguous()
        r1 = ctx.overlap_boxes_device_list(p, capacity=T, stream=s)
        p.zero_()
        o1, i1 = r1.offsets.clone(), r1.ids.clone()
    s.synchronize()
    check((o1.cpu().numpy().view(np.uint64), i1.cpu().numpy()), r, "stream order")
    # n == 0
    e = ctx.overlap_boxes_device_list(torch.empty((0, 8), dtype=torch.float32, device="cuda:0"))
    assert e.offsets.shape == (1,) and int(e.total) == 0 and e.ids is None
    o, i, _ = ctx.overlap_boxes_list(np.zeros((0, 8), np.float32))
    assert o.tolist() == [0] and i is None
    # host forms
    o, i, st = ctx.overlap_boxes_list(boxes, capacity=T)
    check((o, i), r, "host form")
    assert st.node_visits == 0 and st.tri_tests == 0 and st.ms_trace_closest > 0
    o, i, st1 = ctx.overlap_boxes_list(boxes, capacity=0, counting=True)
    assert i is None and o.tobytes() == r[0].tobytes() and st1.node_visits > 0 and st1.tri_tests >= T
    o, i, st2 = ctx.overlap_boxes_list(boxes, capacity=T, counting=True)
    check((o, i), r, "host form, counting")
    # both walks together: the second passes over the records with empty rows and walks the others as the first did
    assert st1.node_visits < st2.node_visits <= 2 * st1.node_visits and st1.tri_tests + T <= st2.tri_tests <= 2 * st1.tri_tests
    o, i, _ = ctx.overlap_boxes_list(boxes)
    check((o, i), r, "host form, capacity=None")
    keep = np.full((T // 2, 2), 0x7F7F7F7F, np.int32)   # the host ids keep what the call does not write
    o = np.zeros(len(boxes) + 1, np.uint64)
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    b32 = np.ascontiguousarray(boxes, np.float32)
    assert ctx.L.rt_overlap_boxes_list(ctx.h, len(boxes), P(b32), 0xFF, 0, P(o), P(keep), T // 2, 0, None) == 0
    assert o.tobytes() == r[0].tobytes() and keep.view(np.uint8).reshape(-1).tobytes() == olr.expected_ids(r[0], r[1], T // 2).tobytes()
    tq = tto.scene_and_sets("small")
    tto.load(ctx, tq[0])
    o, i, _ = ctx.overlap_triangles_list(tq[3]["mixed"])
    check((o, i), tri_csr("small", "mixed"), "triangles, host form")
    c, rsets = ref_sets()
    tst.load(ctx, c.parts)
    o, i, st = ctx.overlap_scene_triangles_list(rsets["others"], counting=True)
    check((o, i), refs_csr("others"), "references, host form")
    assert st.tri_tests > 0


@pytest.mark.gpu
def test_workspace_growth():
    """a small call, then more records, then a larger total on one context: each equals a fresh context's result"""
    parts, sc, tris, sets, ref = tob.scene_and_sets("small")
    boxes = sets["mixed"]
    r = box_csr("small", "mixed")
    big = int(np.argmax(np.diff(r[0].astype(np.int64))))
    steps = [boxes[:40], boxes[:1500], np.concatenate([boxes[:1500], np.repeat(boxes[big:big + 1], 40, axis=0)])]
    c = RtContext(0)
    try:
        tob.load(c, parts)
        grown = [gpu_list(c, "boxes", b, None) for b in steps]
    finally:
        c.close()
    for b, g in zip(steps, grown):
        f = RtContext(0)
        try:
            tob.load(f, parts)
            w = gpu_list(f, "boxes", b, None)
        finally:
            f.close()
        assert g[0].tobytes() == w[0].tobytes() and g[1].tobytes() == w[1].tobytes()
    n0 = int(r[0][1500])
    assert grown[1][1].tobytes() == r[1][:n0].tobytes() and int(grown[2][0][-1]) > 2 * n0


@pytest.mark.gpu
def test_frame_in_flight_beside_a_list_call():
    """a frame of rt_trace_async pending on the context's slot is neither waited for nor changed"""
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
        p = tob.surface_points(sc, 1500, rng, 0.0)
        lo, hi = tob.scene_box(sc)
        h = (hi - lo).max() * 10 ** rng.uniform(-3, -1.0, (1500, 1))
        boxes = tob.as_boxes(p - h, p + h)
        ref = olr.boxes_csr(sc, boxes)
        src = dev("boxes", boxes)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        slot.trace_async(W, H)
        with torch.cuda.stream(s):
            slow_queue(torch, 4)
            res = base.overlap_boxes_device_list(src, capacity=int(ref[0][-1]), stream=s)
        during, _ = slot.trace_wait()
        after = base.trace(W, H)[0]
        s.synchronize()
        assert np.array_equal(during.view(np.uint32), before.view(np.uint32))
        assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
        check(res.numpy(), ref, "beside frames")
        assert np.diff(ref[0].astype(np.int64)).max() > olr.thresholds()[0]
    finally:
        slot.close()
        base.close()


@pytest.mark.gpu
def test_error_statuses():
    import torch
    from tests import scenes
    from tests.test_ray_query import PATHS
    sp = scenes.two_object_scene(PATHS[0], PATHS[1], 1, 0, 2, 1, ctx=None)
    sc = cr.Scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, sp.instances)
    rng = np.random.default_rng(121)
    pts = tob.surface_points(sc, 500, rng, 0.0)
    boxes_np = tob.as_boxes(pts - 0.01, pts + 0.01)
    ref = olr.boxes_csr(sc, boxes_np)
    T = int(ref[0][-1])
    boxes = dev("boxes", boxes_np)
    n = boxes.shape[0]
    off = torch.empty((n + 2,), dtype=torch.int64, device="cuda:0")
    ids = torch.empty((T + 2, 2), dtype=torch.int32, device="cuda:0")
    B_, O_, I_ = boxes.data_ptr(), off.data_ptr(), ids.data_ptr()
    c = RtContext(0)
    p = lambda x: ctypes.c_void_p(x) if x else None   # noqa: E731

    def raw(name, n_, rec, cull, flags, o, i, cap):
        return getattr(c.L, "rt_overlap_%s_device_list" % name)(c.h, n_, p(rec), cull, flags, p(o), p(i), cap, None)

    def err(args, code, text, name="boxes"):
        assert raw(name, *args) == code, args
        msg = c.L.rt_last_error(c.h).decode()
        assert text in msg, (args, msg)

    def ok():
        check(gpu_list(c, "boxes", boxes_np, T), ref, "after a refused call")

    try:
        err((n, B_, 0xFF, 0, O_, I_, T), RT_ERR_NOT_READY, "")   # no geometry
        c.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        err((n, B_, 0xFF, 0, O_, I_, T), RT_ERR_NOT_READY, "")   # no TLAS
        c.set_instances(sp.instances)
        c.set_uniforms(sp.uniforms)
        ok()
        bad = [((n, B_, 0xFF, 0, O_ + 4, I_, T), "aligned"), ((n, B_, 0xFF, 0, O_, I_ + 2, T), "aligned"), ((n, B_ + 4, 0xFF, 0, O_, I_, T), "aligned"),
               ((n, B_, 0xFF, 0x1, O_, I_, T), "RT_OVERLAP_ANY"), ((n, B_, 0xFF, 0x1, O_, 0, 0), "RT_OVERLAP_ANY"), ((n, B_, 0xFF, 0x2, O_, I_, T), "unknown flag bits"),
               ((n, B_, 0xFF, 0x80000000, O_, I_, T), "unknown flag bits"), ((n, B_, 0xFF, 0, O_, 0, T), "null id pointer"), ((n, B_, 0xFF, 0, O_, I_, 0), "capacity 0"),
               ((0xFFFFFF00, B_, 0xFF, 0, O_, I_, T), "too many boxes"), ((n, B_, 0xFF, 0, O_, I_, 0xFFFFFF00), "capacity must be below"),
               ((n, B_, 0x100, 0, O_, I_, T), "cull_mask"), ((n, 0, 0xFF, 0, O_, I_, T), "null record/offset"), ((n, B_, 0xFF, 0, 0, I_, T), "null record/offset")]
        host_buf = np.zeros((n + 1, 8), np.float32)
        pinned = torch.zeros((n, 8), dtype=torch.float32).pin_memory()
        for ptr in ((host_buf.ctypes.data + 15) & ~15, pinned.data_ptr()):   # (16-byte aligned: only the memory kind is wrong)
            bad += [((n, ptr, 0xFF, 0, O_, I_, T), "device memory of the context's GPU"), ((n, B_, 0xFF, 0, ptr, I_, T), "device memory of the context's GPU"),
                    ((n, B_, 0xFF, 0, O_, ptr, T), "device memory of the context's GPU")]
        for args, text in bad:
            err(args, RT_ERR_INVALID_ARGUMENT, text)
            ok()
        for name in NAMES[1:]:   # the other two calls share the checker
            err((n, B_, 0xFF, 0x1, O_, I_, T), RT_ERR_INVALID_ARGUMENT, "RT_OVERLAP_ANY", name)
            err((n, B_, 0xFF, 0, O_ + 4, I_, T), RT_ERR_INVALID_ARGUMENT, "aligned", name)
            err((n, B_, 0xFF, 0, O_, I_, 0xFFFFFF00), RT_ERR_INVALID_ARGUMENT, "capacity must be below", name)
        # 8-byte aligned offsets and 4-byte aligned ids that are not 16-byte aligned are fine
        assert raw("boxes", n, B_, 0xFF, 0, O_ + 8, I_ + 4, T) == 0
        torch.cuda.synchronize()
        assert off[1:].cpu().numpy().view(np.uint64).tobytes() == ref[0].tobytes()
        assert ids.view(-1)[1:1 + 2 * T].cpu().numpy().tobytes() == ref[1].tobytes()
        o = np.zeros(n + 1, np.uint64)
        P = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        h_ids = np.zeros((T, 2), np.int32)
        assert c.L.rt_overlap_boxes_list(c.h, n, None, 0xFF, 0, P(o), P(h_ids), T, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_overlap_boxes_list(c.h, n, P(boxes_np), 0x100, 0, P(o), P(h_ids), T, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_overlap_boxes_list(c.h, n, P(boxes_np), 0xFF, 1, P(o), None, 0, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_overlap_boxes_list(c.h, n, P(boxes_np), 0xFF, 0, P(o), None, T, 0, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_overlap_boxes_list(c.h, n, P(boxes_np), 0xFF, 0, None, None, 0, 0, None) == RT_ERR_INVALID_ARGUMENT
        ok()
        assert raw("boxes", 0, 0, 0xFF, 0, 0, 0, 0) == 0   # n == 0 enqueues nothing and needs no pointers
        with pytest.raises(ValueError):
            c.overlap_boxes_device_list(boxes.cpu())
        with pytest.raises(ValueError):
            c.overlap_boxes_device_list(torch.zeros((4, 4), dtype=torch.float32, device="cuda:0"))
        with pytest.raises(RtError) as e:
            c.overlap_boxes_device_list(boxes, capacity=T, cull_mask=0x1FF)
        assert e.value.code == RT_ERR_INVALID_ARGUMENT
        ok()
    finally:
        c.close()
    a = RtContext(0, variant="alt")   # trace_variant != 0 (alt library only: the product refuses the parameter itself)
    try:
        a.set_param("blas_builder", 0)
        a.set_param("trace_variant", 1)
        a.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        a.set_instances(sp.instances)
        c = a
        err((n, B_, 0xFF, 0, O_, I_, T), RT_ERR_INVALID_ARGUMENT, "trace_variant 0")
        a.set_param("trace_variant", 0)
        a.set_instances(sp.instances)
        ok()
    finally:
        a.close()


@pytest.mark.gpu
def test_offsets_beyond_32_bits(ctx):
    """ceil(2^32 / M) + 16 copies of the enclosing box of the teapot scene (M: its admitted finite triangles, confirmed by the brute
    force on one box), offsets only: offsets[i] == i * M exactly, the last ones above 2^32.  About 4.3e9 predicate evaluations and no id
    traffic.  On the teapot scene M = 11 280 and n = 380 776; the whole test, the 12 MB of boxes and the comparison included, took
    0.07 s on an MI355X."""
    import torch
    parts, sc, tris, sets, ref = tob.scene_and_sets("teapot")
    tob.load(ctx, parts)
    lo, hi = tob.scene_box(sc)
    box = tob.as_boxes(lo[None] - 1, hi[None] + 1)
    M = int(olr.boxes_csr(sc, box, tris=tris)[0][-1])
    assert M == int((tris.finite & sc.admitted(0xFF)).sum()) > 1000
    n = -(-(1 << 32) // M) + 16
    src = dev("boxes", box).expand(n, 8).contiguous()
    res = ctx.overlap_boxes_device_list(src, capacity=0)
    torch.cuda.synchronize()
    want = torch.arange(n + 1, dtype=torch.int64, device="cuda:0") * M
    assert res.ids is None and int(res.total) == n * M > (1 << 32)
    assert torch.equal(res.offsets, want)
