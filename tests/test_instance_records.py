"""Bad instance records (include/rt_api.h at rt_set_instances; DESIGN.md §5 "Instance records"): one must not cost the scene its other hits.

tests/instance_record_cases.py holds the case table (void, non-invertible and far records), the scenes (1, 2, 5 and 300 records), the
twin of a scene (the bad records masked out, their transforms the identity) and the query records.  The CPU part holds the inputs to
conditions that "everything misses" or "nothing changed" cannot meet, the case table to the contract's own definition of its classes,
and the host builder to a clean run under the sanitizers.  The GPU part runs every (producer, class): the five producers of a TLAS
(rt_set_instances build and update, rt_set_instances_device build and refit, rt_set_batch with the bad record in frame 1 only), all
consumers in each — closest and any hits, flags with attributes, the 4 nearest hits with counts, closest points, sphere sweeps, box and
triangle overlaps, point-inside votes, signed distances, shaded rays, a frame with the default tunables and one without coverage mask
and pixel beams:
  * against the references (the two build producers): the oracle given the TWIN records for the ray consumers and the frame — closest
    hits, blocked segments, flags and hit kinds, the four nearest candidates and their number (oracle_lists of
    tests/test_ray_query_hits.py), the crossing counts and vote words of every point (tests/inside_reference.py), the shaded samples
    and point averages (tests/shade_reference.py), the frames; the binary32 restatements of tests/closest_reference.py,
    sweep_reference.py, overlap_reference.py and triangle_overlap_reference.py for the world-space consumers — given the twin for void
    and far records, the records as they are for non-invertible ones — byte for byte, as the tests of those consumers compare them;
  * in every producer and class the signed distance is that run's closest point with the sign of that run's vote word
    (tests/test_point_inside.py), so with the words held to the oracle over the twin its vote never counts a bad record; for a
    non-invertible record under the update and refit producers the world-space buffers equal a plain host build's over the same records;
  * against the twin on the same library: every output buffer byte-identical to the twin scene's (for a non-invertible record the
    ray consumers' buffers: the world-space consumers keep its o2w image, which the twin does not have; of the any-hit query whether
    each segment is blocked: which blocker a walk meets first depends on the tree, tests/test_device_tlas.py);
  * the tree: rt_debug_snapshot passes tests/tree_reference.py, which knows a void record (mask word 0, BOX_NONE, out of the bounds).
"""
import os
import subprocess

import numpy as np
import pytest

from tests import closest_reference as cr
from tests import consumers
from tests import inside_reference as ir
from tests import instance_record_cases as irc
from tests import overlap_reference as orf
from tests import sweep_reference as sr
from tests import tree_reference as tr
from tests import triangle_overlap_reference as tor
from tests.consumers import assert_same, check_signed_distance, dev
from tests.exact import assert_frame_equals_oracle, assert_hits_equal_oracle
from tests.shade_reference import average_points, shade_samples
from tests.test_ray_query_hits import oracle_lists
from vulkan_raytracing_amd import RtContext, api, tiling
from vulkan_raytracing_amd.api import INSTANCE_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = irc.FRAME_W, irc.FRAME_H
RAY_CONSUMERS, WORLD_CONSUMERS = consumers.RAY_CONSUMERS, consumers.WORLD_CONSUMERS


def cases():
    return [(cls, case) for cls, table in irc.CLASSES.items() for case in table]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------

def oracle_hits(name, records):
    sp = irc.scene(name)
    sp.orc.set_instances([records[i].tobytes() for i in range(len(records))])
    try:
        return sp.orc.intersect(irc.probe_rays(name))
    finally:
        sp.orc.set_instances([sp.instances[i].tobytes() for i in range(len(sp.instances))])


@pytest.mark.parametrize("name", list(irc.SCENES))
def test_probe_rays_meet_the_conditions(name):
    """conditions on the inputs, against the oracle alone: in the twin at least 40 % of the rays hit; for n >= 5 at least 25 % hit an
    instance with a larger index than the bad record and at least 25 % one with a smaller index; in the unmodified scene at least 10
    rays hit the record that is about to be made bad.  (n = 1 has no twin hits: its only record is the bad one.)"""
    n, _, bad = irc.SCENES[name]
    sp = irc.scene(name)
    good = oracle_hits(name, sp.instances)
    twin = oracle_hits(name, irc.twin_records(sp.instances, [bad]))
    share = (twin["inst"] >= 0).mean()
    larger, smaller = (twin["inst"] > bad).mean(), ((twin["inst"] >= 0) & (twin["inst"] < bad)).mean()
    on_bad = int((good["inst"] == bad).sum())
    print("%s: twin hit share %.1f %%, larger / smaller index %.1f %% / %.1f %%, rays that hit the bad record %d" % (name, 100 * share, 100 * larger, 100 * smaller, on_bad))
    assert on_bad >= 10
    assert not (twin["inst"] == bad).any()
    if n >= 2:
        assert share >= 0.40
    else:
        assert share == 0.0
    if n >= 5:
        assert larger >= 0.25 and smaller >= 0.25


def classify(records, ranges_lo_hi):
    """the contract's definition in numpy (tests/tree_reference.py padded_world_box): 'void', 'noninvertible' or 'ok' per record"""
    t = np.asarray(records["transform"], np.float32).reshape(-1, 12)
    lo = np.array([ranges_lo_hi[int(m)][0] for m in records["mesh"]], np.float32)
    hi = np.array([ranges_lo_hi[int(m)][1] for m in records["mesh"]], np.float32)
    blo, bhi = tr.padded_world_box(t, lo, hi)
    out = []
    for i in range(len(t)):
        with np.errstate(all="ignore"):
            inside = bool((np.abs(blo[i]) < tr.INST_BOX_LIMIT).all() and (np.abs(bhi[i]) < tr.INST_BOX_LIMIT).all())
            w2o = cr.world_to_object(t[i])
        out.append("void" if not (np.isfinite(t[i]).all() and inside) else "ok" if np.isfinite(w2o).all() else "noninvertible")
    return out


def mesh_bounds(sp):
    pos = sp.geom.verts.reshape(-1, 6)[:, :3]
    out = []
    for ff, fi, pc in sp.geom.ranges:
        v = sp.geom.verts[ff:].reshape(-1, 6)[np.unique(sp.geom.idx[fi:fi + 3 * pc]), :3]
        out.append((v.min(axis=0), v.max(axis=0)))
    return out


@pytest.mark.parametrize("name", list(irc.SCENES))
def test_every_case_is_of_its_class(name):
    """by the contract's own definition every case of the table makes a record of its class out of a good one, on every scene; far
    records and the records the case leaves alone are valid ones"""
    sp = irc.scene(name)
    mb = mesh_bounds(sp)
    assert set(classify(sp.instances, mb)) == {"ok"}
    for cls, case in cases():
        fns = irc.CLASSES[cls][case]
        bad = irc.bad_indices(name, fns)
        got = classify(irc.bad_records(sp.instances, name, fns), mb)
        want = "ok" if cls == "far" else cls
        assert [got[i] for i in bad] == [want] * len(bad) and all(g == "ok" for i, g in enumerate(got) if i not in bad), (name, case, got[:8])
    assert len(irc.bad_indices("n300", irc.VOID["nan_slots"])) == 12
    t = irc.bad_records(irc.scene("n300").instances, "n300", irc.VOID["nan_slots"])["transform"][150:162]
    assert np.array_equal(np.argwhere(np.isnan(t)), np.stack([np.arange(12), np.arange(12)], axis=1))   # record 150 + k: NaN in slot k only
    ff = irc.bad_records(sp.instances, name, irc.VOID["bytes_ff"])[irc.SCENES[name][2]]
    assert ff["transform"].tobytes() == b"\xff" * 48 and ff["mesh"] == sp.instances[irc.SCENES[name][2]]["mesh"] and int(ff["custom_index_and_mask"]) >> 24 == 0xFF


def test_host_builder_is_clean_under_the_sanitizers():
    """`make sanitize-builder`: tests/native/builder_sanitize.cpp links csrc/bvh_build.cpp and runs build_bvh, refit_bvh, collapse_bvh4
    and quantize_bvh2 over infinite, inverted, absent and NaN boxes at 1, 2, 300 and 5000 boxes under AddressSanitizer and UBSan with
    float-cast-overflow (a stand-alone host program: no GPU, nothing preloaded)"""
    r = subprocess.run(["make", "-C", ROOT, "sanitize-builder"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "0 failures" in r.stdout and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

def load(name):
    """a context of its own with the scene's geometry, uniforms and sky, and the good records set"""
    c = RtContext(0)
    try:
        return c, irc.scene(name, ctx=c)
    except BaseException:
        c.close()
        raise


def consume(c, name):
    """every consumer once over the scene's query records -> {buffer name: numpy array} (tests/consumers.py)"""
    return consumers.consume(c, irc.probe_rays(name), irc.query_records(name), 3 * irc.SCENES[name][1] + 10, W, H)


def consume_world(c, name):
    return consumers.consume_world(c, irc.query_records(name))


_BUILT = {}


def built_world(name, case, records):
    """the world-space consumers' buffers over `records` under a plain host build in a context of its own (cached): what the update,
    refit and batch-free producers must reproduce for a non-invertible record, whose o2w image the twin does not have"""
    if (name, case) not in _BUILT:
        c, _ = load(name)
        try:
            c.set_instances(records)
            _BUILT[(name, case)] = consume_world(c, name)
        finally:
            c.close()
    return _BUILT[(name, case)]


_TWIN = {}


def twin_outputs(name, n_bad=1):
    """the twin scene's buffers (host build), once per scene and number of bad records"""
    key = (name, n_bad)
    if key not in _TWIN:
        c, sp = load(name)
        try:
            bad = irc.bad_indices(name, (None,) * n_bad)
            c.set_instances(irc.twin_records(sp.instances, bad))
            _TWIN[key] = consume(c, name)
        finally:
            c.close()
    return _TWIN[key]


N_LISTS, N_VOTE = irc.N_RAYS, irc.N_RECORDS   # rays whose four nearest hits, and points whose crossing counts, the oracle restates: all
_RAY_REF = {}


def ray_references(name, orc, key, twin):
    """oracle references over the twin records that cost a pass over every triangle, once per twin: the 4 nearest candidates and their
    number (tests/test_ray_query_hits.py oracle_lists) of the first N_LISTS rays, the crossing counts (tests/inside_reference.py) of
    the first N_VOTE points, the shaded samples and point averages of every ray (tests/shade_reference.py)"""
    if key not in _RAY_REF:
        sp = irc.scene(name)
        rays = irc.probe_rays(name)
        orc.tri_counts = ir.tri_counts(sp.geom.ranges, twin)
        n_points = len(rays) // 2
        s = shade_samples(orc, rays, n_points, int(sp.uniforms[0]["max_bounce_count"]))
        _RAY_REF[key] = dict(lists=oracle_lists(orc, rays[:N_LISTS], None, 0, 0xFF, 4),
                             counts=ir.oracle_counts(orc, orc.tri_counts, irc.query_records(name)["points"][:N_VOTE], 3),
                             shade_s=s, shade_p=average_points(s, n_points, 2))
    return _RAY_REF[key]


_REF = {}


def subset(name):
    """128 of the query records: those aimed at the scene's bad record first (every n-th), then the others in order"""
    n, _, bad = irc.SCENES[name]
    i = np.arange(irc.N_RECORDS)
    return np.concatenate([i[i % n == bad], i[i % n != bad]])[:128]


def world_references(name, records, key, sel=None):
    """brute32 of the four world-space consumers over `records` (cached by key), for the query records `sel` (all of them: None)"""
    if key not in _REF:
        sp = irc.scene(name)
        q = {k: (v if sel is None else v[sel]) for k, v in irc.query_records(name).items()}
        with np.errstate(all="ignore"):
            sc = cr.Scene(sp.geom.verts, sp.geom.idx, sp.geom.ranges, records)
            tris = orf.Triangles(sc)
            _REF[key] = dict(sc=sc, cp=cr.brute32(sc, q["points"]), sweep=sr.brute32(sc, q["sweeps"]), boxes=orf.brute32(sc, q["boxes"], max_ids=16, tris=tris),
                             tris=tor.brute32(sc, q["tris"], max_ids=16, tris=tris))
    return _REF[key]


def check_references(name, got, twin, ray_key, world_records, world_key, sel=None):
    """the ray consumers and the frame against the oracle over the twin records; the world-space consumers against their restatements"""
    sp = irc.scene(name)
    orc = sp.orc
    orc.set_instances([twin[i].tobytes() for i in range(len(twin))])
    try:
        rays = irc.probe_rays(name)
        assert_hits_equal_oracle(got["closest"].view(api.HIT_DTYPE).reshape(-1), orc, rays)
        sh = rays.copy(); sh[:, 7] = 3 * irc.SCENES[name][1] + 10
        assert np.array_equal(got["any"], orc.intersect(sh, any_hit=True)["inst"] >= 0), name
        ref, kinds = orc.intersect_query(rays, ray_flags=api.RAY_FLAG_CULL_BACK_FACING)
        assert got["flags"].tobytes() == ref.tobytes(), name
        assert np.array_equal(got["flags_attr"][:, 7].view(np.uint32), kinds), name
        lists = got["hits4"].view(api.HIT_DTYPE).reshape(len(rays), 4)
        assert lists[:, 0]["t"].tobytes() == orc.intersect_query(rays)[0]["t"].tobytes(), name   # the nearest of the four lies at the closest hit's t
        rr = ray_references(name, orc, ray_key, twin)
        rh, _, rcount = rr["lists"]
        assert lists[:N_LISTS].tobytes() == rh.tobytes() and np.array_equal(got["hits4_count"][:N_LISTS].view(np.uint32), rcount), name
        assert np.array_equal(got["inside_count"][:N_VOTE].view(np.uint32), rr["counts"]), name
        assert np.array_equal(got["inside"][:N_VOTE].view(np.uint32), ir.words(rr["counts"], 3, True)), name
        for k in ("shade_s", "shade_p"):
            assert np.array_equal(got[k].view(np.uint32), rr[k].view(np.uint32)), (name, k)
        ref_img, rc = orc.render(W, H)
        for key in ("frame", "frame_plain"):
            assert_frame_equals_oracle(got[key], orc, W, H, ref=ref_img)
            assert tuple(got[key + "_counts"]) == tuple(int(x) for x in rc), key
    finally:
        orc.set_instances([sp.instances[i].tobytes() for i in range(len(sp.instances))])
    if world_records is None:
        return None
    ref = world_references(name, world_records, world_key, sel)
    rows = slice(None) if sel is None else sel
    assert got["cp"].view(api.HIT_DTYPE).reshape(-1)[rows].tobytes() == ref["cp"].tobytes(), (name, world_key)
    assert got["sweep"].view(api.HIT_DTYPE).reshape(-1)[rows].tobytes() == ref["sweep"].tobytes(), (name, world_key)
    for k in ("boxes", "tris"):
        rc_, ri = ref[k]
        assert got[k + "_count"][rows].astype(rc_.dtype).tobytes() == rc_.tobytes(), (name, world_key, k)
        assert got[k + "_ids"][rows].astype(ri.dtype).tobytes() == np.ascontiguousarray(ri[:, :16]).tobytes(), (name, world_key, k)
    return ref


def validate(c, records, what):
    """the context's snapshot passes the validator; its meshes are walked once per context (instances do not change them)"""
    snap = c.debug_snapshot()
    viol, _ = tr.validate(snap, np.asarray(records["mesh"], np.int64).reshape(-1), blas=not getattr(c, "_blas_validated", False))
    c._blas_validated = True
    assert {k: v for k, v in viol.items() if v} == {}, (what, {k: v for k, v in viol.items() if v})
    return snap


def world_too(cls, name):
    """are the world-space consumers held to the twin?  Not for a non-invertible record (they keep its o2w image).  Not for a far record
    that is the scene's only one: nothing is promised about hitting the record itself, a closest-point query of infinite radius finds it
    1e30 away when there is nothing else, and there is no rest of the scene to answer as before."""
    return cls == "void" or (cls == "far" and irc.SCENES[name][0] > 1)


def keys_of(cls, name):
    return RAY_CONSUMERS + (WORLD_CONSUMERS if world_too(cls, name) else ())


def run_class(producer, cls, scene_names=tuple(irc.SCENES)):
    import torch
    on_bad = 0   # reference answers of the world-space consumers that lie on a non-invertible record's image
    for name in scene_names:
        c, sp = load(name)
        try:
            good = sp.instances
            first = None
            if producer == "device_refit":
                c.set_instances_device(dev(good.view(np.uint8).reshape(-1, 64), np.uint8))
                first = c.debug_snapshot()
            for case, fns in irc.CLASSES[cls].items():
                what = "%s, %s, %s" % (producer, name, case)
                bad = irc.bad_records(good, name, fns)
                idx = irc.bad_indices(name, fns)
                twin = irc.twin_records(good, idx)
                if producer == "host_build":
                    c.set_instances(bad)
                elif producer == "host_update":
                    c.set_instances(good)
                    c.set_instances(bad, update=True)
                elif producer == "device_build":
                    c.set_instances_device(dev(bad.view(np.uint8).reshape(-1, 64), np.uint8))
                elif producer == "device_refit":
                    c.set_instances_device(dev(bad.view(np.uint8).reshape(-1, 64), np.uint8), update=True)
                got = consume(c, name)
                assert_same(got, twin_outputs(name, len(idx)), keys_of(cls, name), what)
                validate(c, bad, what)
                check_signed_distance(got, what)
                if producer in ("host_build", "device_build"):
                    if cls == "noninvertible":   # the world-space consumers keep the o2w image: the records as they are, 128 query records
                        ref = check_references(name, got, twin, (name, len(idx)), bad, (name, case), subset(name))
                        on_bad += int((ref["cp"]["inst"] == idx[0]).sum()) + int((ref["sweep"]["inst"] == idx[0]).sum())
                    else:
                        check_references(name, got, twin, (name, len(idx)), twin if world_too(cls, name) else None, (name, "twin", len(idx)))
                elif cls == "noninvertible":
                    # the twin lacks the o2w image: the world-space buffers are the plain host build's over the same records
                    assert_same(got, built_world(name, case, bad), WORLD_CONSUMERS, what, "the host build's")
                if producer == "device_refit":
                    # a second refit turns the record good again: that state equals the original bit for bit
                    c.set_instances_device(dev(good.view(np.uint8).reshape(-1, 64), np.uint8), update=True)
                    again = c.debug_snapshot()
                    for k in ("instances", "tlas_nodes", "tlas_q_lo", "tlas_q_scale"):
                        assert again[k].tobytes() == first[k].tobytes(), (what, k)
            torch.cuda.synchronize()
        finally:
            c.close()
    if cls == "noninvertible" and producer in ("host_build", "device_build"):
        assert on_bad >= 10, on_bad   # (the image is there to be found: the references found it)


@pytest.mark.gpu
def test_nan_translation_of_one_of_two_records_closest_hits():
    """the smallest case on its own: n = 2, host build, a NaN translation, closest hits only — the twin's hits, and the oracle's over
    the twin records"""
    import torch
    name = "n2_first"
    c, sp = load(name)
    try:
        rays = irc.probe_rays(name)
        bad = irc.bad_records(sp.instances, name, (irc.VOID["nan_slots"][3],))
        twin = irc.twin_records(sp.instances, [0])
        c.set_instances(bad)
        got = c.intersect_device(dev(rays)).hits
        c.set_instances(twin)
        want = c.intersect_device(dev(rays)).hits
        torch.cuda.synchronize()
        got, want = got.cpu().numpy(), want.cpu().numpy()
        assert got.tobytes() == want.tobytes()
        hits = got.view(api.HIT_DTYPE).reshape(-1)
        assert (hits["inst"] == 1).mean() >= 0.4 and not (hits["inst"] == 0).any()
        sp.orc.set_instances([twin[i].tobytes() for i in range(2)])
        try:
            assert_hits_equal_oracle(hits, sp.orc, rays)
        finally:
            sp.orc.set_instances([sp.instances[i].tobytes() for i in range(2)])
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cls", list(irc.CLASSES))
@pytest.mark.parametrize("producer", ["host_build", "host_update", "device_build", "device_refit"])
def test_a_bad_record_costs_the_scene_nothing(producer, cls):
    run_class(producer, cls)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", list(irc.CLASSES))
def test_a_bad_record_in_frame_1_of_a_batch(cls):
    """rt_set_batch with K = 2 and the bad record in frame 1 only: both frames equal the twin batch's, frame 0 as well (the frames
    share one quantisation), and both trees validate.  Queries are RT_ERR_NOT_READY on a batch: only the frames run."""
    import torch
    band, rows = 8, tiling.max_shard_rows(H, 8, 1)

    def batch(c, sp, second):
        c.set_batch(np.stack([sp.instances, second]), np.concatenate([sp.uniforms, sp.uniforms]))
        buf = torch.zeros((2, rows, W, 4), dtype=torch.float32, device="cuda:0")
        c.trace_shard_batch(W, H, band, 0, 1, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream, frame_stride_bytes=rows * W * 16)
        st = c.stats()
        return buf.cpu().numpy(), (st.rays_primary, st.rays_secondary, st.rays_shadow)

    for name in irc.SCENES:
        c, sp = load(name)
        try:
            twins = {}
            for case, fns in irc.CLASSES[cls].items():
                what = "batch, %s, %s" % (name, case)
                idx = irc.bad_indices(name, fns)
                if len(idx) not in twins:
                    twins[len(idx)] = batch(c, sp, irc.twin_records(sp.instances, idx))
                bad = irc.bad_records(sp.instances, name, fns)
                got = batch(c, sp, bad)
                validate(c, np.concatenate([sp.instances, bad]), what)
                assert got[0].tobytes() == twins[len(idx)][0].tobytes() and got[1] == twins[len(idx)][1], what
        finally:
            c.close()
