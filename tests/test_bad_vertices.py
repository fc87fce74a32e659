"""Bad vertex positions (include/rt_api.h at rt_upload_geometry; DESIGN.md §5 "Bad vertices"): one must not cost the mesh.

A triangle with a position coordinate that is not finite or of magnitude >= 1e37 is inactive in every builder and for every consumer;
every other triangle keeps its primitive index and its answers, bit for bit.  tests/bad_vertex_cases.py holds the case table (coordinate
classes, patterns, meshes), the twin of a mesh (the bad triangles pointed at one all-NaN vertex: only the oracle and the references
ever see it), the scene and the query records.

The CPU part holds the oracle to the twin on the non-finite classes, the inputs to conditions that "everything misses" or "nothing
changed" cannot meet, the host builder's trees of every (class, pattern, mesh) to the node-by-node validator and to
rt_debug_check_builders, the threaded host build to the single-threaded one, and the host builder to a clean run under the sanitizers.
The GPU part runs every producer of a BLAS (rt_build_blas on the host and with the three device builders, rt_build_blas after a refit
that left the bad vertices on the device only, a good refit over a mesh built with inactive triangles) and every consumer
(tests/consumers.py), byte for byte against the oracle and the binary32 brute forces over the twin (the far classes: over the vertices
as they are), and the snapshot of every producer against the validator.  No comparison has a tolerance."""
import os
import subprocess

import numpy as np
import pytest

from tests import bad_vertex_cases as bv
from tests import closest_reference as cr
from tests import consumers
from tests import inside_reference as ir
from tests import overlap_reference as orf
from tests import sweep_reference as sr
from tests import tree_reference as tr
from tests import triangle_overlap_reference as tor
from tests.shade_reference import average_points, shade_samples
from tests.test_ray_query_hits import oracle_lists
from tests.test_tree_invariants import clean, use_builder
from vulkan_raytracing_amd import RtContext, api
from vulkan_raytracing_amd.api import RtError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = bv.FRAME_W, bv.FRAME_H
ANY_TMAX = 25.0
RT_ERR_INVALID_ARGUMENT = 1
# the classes the other patterns and meshes run with (a NaN, an infinite vertex, the limit itself, the far number below it; on the
# teapot the triangle with +inf and -inf as well)
OTHER_CLASSES = {"teapot": ("nan_y", "ninf_vertex", "inf_pm", "1e37_y", "below_1e37_y")}
SMALL_CLASSES = ("nan_y", "ninf_vertex", "1e37_y", "below_1e37_y")
OTHER_CASES = [("teapot", p) for p in ("one", "first_third", "all", "duplicate")] + \
              [(m, p) for m in ("tri9", "tri8", "tri7", "soup") for p in ("every40", "first_third", "all")]


def rows_differ(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return (a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1)


# ---- CPU: the oracle and the references ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cls", list(bv.BAD))
def test_oracle_on_bad_vertices(cls):
    """non-finite classes: the oracle over the vertices as they are equals the oracle over the twin byte for byte, by brute force and
    with its BVH — no ray hits a bad triangle.  3e38 and 1e37: they differ (rays hit the huge triangles): there the contract departs
    from the oracle, and the twin is the reference."""
    for pattern in ("every40", "one"):
        sc = bv.scene("teapot", cls, pattern)
        rays = bv.rays(sc)
        twin, asis = bv.oracle_scene(sc, True), bv.oracle_scene(sc, False)
        want = twin.intersect(rays)
        assert twin.intersect(rays, use_bvh=False).tobytes() == want.tobytes()
        bad = sc["m"]["bad"]
        assert not (bad[np.clip(want["prim"], 0, len(bad) - 1)] & (want["inst"] >= 0) & (want["inst"] < 2)).any()
        got = [asis.intersect(rays), asis.intersect(rays, use_bvh=False)]
        if cls in bv.NON_FINITE:
            assert got[0].tobytes() == want.tobytes() and got[1].tobytes() == want.tobytes(), (cls, pattern)
        else:
            n = int(rows_differ(got[1], want).sum())
            print("%s, %s: %d of %d rays answer differently over the vertices as they are" % (cls, pattern, n, len(rays)))
            assert n > 0, (cls, pattern)


def _bad_sets():
    """every (mesh, pattern) the GPU part runs, with one class of each set of bad triangles (inf_pm touches a second vertex)"""
    return [("teapot", "every40", c) for c in ("nan_y", "inf_pm")] + [(m, p, "nan_y") for m, p in OTHER_CASES]


@pytest.mark.parametrize("name,pattern,cls", _bad_sets())
def test_rays_meet_the_conditions(name, pattern, cls):
    """on the oracle alone.  Patterns every40 and first_third: at least half the rays hit in the twin and at least 2 % answer differently
    than on the clean mesh (both over the random part alone as well on the teapot).  Patterns one and duplicate: of the aimed rays at
    least 100 pass through a bad triangle of instance 0 and hit something behind it (duplicate: the good triangle it coincides with).
    Pattern all: no ray hits the mesh, and the cube is still hit."""
    sc = bv.scene(name, cls, pattern)
    rays, m = bv.rays(sc), sc["m"]
    twin = bv.oracle_scene(sc, True).intersect(rays)
    good = bv.oracle_scene(sc, True, clean_mesh=True).intersect(rays)
    changed = rows_differ(twin, good)
    through = (good["inst"] == 0) & m["bad"][np.clip(good["prim"], 0, len(m["bad"]) - 1)] & (twin["inst"] >= 0)
    share, aimed = (twin["inst"] >= 0).mean(), slice(bv.N_RANDOM, None)
    print("%s %s %s: %d bad of %d; twin hit share %.1f %%, changed %.1f %%, aimed rays through a bad triangle with a hit behind %d" %
          (name, pattern, cls, m["bad"].sum(), len(m["bad"]), 100 * share, 100 * changed.mean(), through[aimed].sum()))
    assert not ((twin["inst"] < 2) & (twin["inst"] >= 0) & m["bad"][np.clip(twin["prim"], 0, len(m["bad"]) - 1)]).any()
    if pattern == "all":
        assert m["bad"].all() and not (twin["inst"] == 0).any() and not (twin["inst"] == 1).any() and (twin["inst"] == 2).sum() >= 100
        return
    if pattern in ("every40", "first_third"):
        assert share >= 0.5 and changed.mean() >= 0.02
        if name == "teapot":
            assert (twin["inst"][:bv.N_RANDOM] >= 0).mean() >= 0.5 and changed[:bv.N_RANDOM].mean() >= 0.02
    if pattern == "duplicate":
        original = (len(m["bad"]) - 1) // 2
        assert m["bad"].sum() == 1 and m["bad"][-1] and ((twin["inst"] == 0) & (twin["prim"] == original))[aimed].sum() >= 100
    else:
        assert through[aimed].sum() >= 100


def world_scene(sc, twin, n_inst=4, verts=None):
    return cr.Scene(sc["verts"] if verts is None else verts, sc["twin_idx"] if twin else sc["idx"], sc["ranges"], bv.instances(n_inst))


def world_brute(scene_, q):
    with np.errstate(all="ignore"):
        tris = orf.Triangles(scene_)
        return dict(cp=cr.brute32(scene_, q["points"]), sweep=sr.brute32(scene_, q["sweeps"]), boxes=orf.brute32(scene_, q["boxes"], max_ids=16, tris=tris),
                    tris=tor.brute32(scene_, q["tris"], max_ids=16, tris=tris))


@pytest.mark.parametrize("name,pattern,cls", [("teapot", "every40", "nan_y"), ("teapot", "first_third", "nan_y"), ("soup", "every40", "nan_y")])
def test_query_records_meet_the_conditions(name, pattern, cls):
    """the same two conditions for the points, sweeps, boxes and query triangles, on the binary32 brute forces alone: at least half of
    each have an answer in the twin, at least 2 % answer differently than on the clean mesh"""
    sc = bv.scene(name, cls, pattern)
    q = bv.query_records(sc)
    twin = world_brute(world_scene(sc, True), q)
    cv = sc["verts"].copy()
    cv[:sc["ranges"][1][0]].reshape(-1, 6)[sc["m"]["idx"].astype(np.int64), :3] = sc["m"]["clean"].reshape(-1, 3)
    good = world_brute(world_scene(sc, False, verts=cv), q)
    for k in ("cp", "sweep"):
        share, ch = (twin[k]["inst"] >= 0).mean(), rows_differ(twin[k], good[k]).mean()
        print("%s %s, %s: %.1f %% answered in the twin, %.1f %% changed" % (name, pattern, k, 100 * share, 100 * ch))
        assert share >= 0.5 and ch >= 0.02, k
    for k in ("boxes", "tris"):
        share = (twin[k][0] > 0).mean()
        ch = (rows_differ(twin[k][0].reshape(-1, 1), good[k][0].reshape(-1, 1)) | rows_differ(twin[k][1], good[k][1])).mean()
        print("%s %s, %s: %.1f %% answered in the twin, %.1f %% changed" % (name, pattern, k, 100 * share, 100 * ch))
        assert share >= 0.5 and ch >= 0.02, k


# ---- CPU: the host builder ------------------------------------------------------------------------------------------------------------

def host_part(m):
    rc, hb = api.host_blas(m["verts"], m["idx"])
    rc2, st = api.check_builders(m["verts"], m["idx"])
    assert rc == 0, rc
    return (m["verts"], m["idx"], hb["nodes"], hb["packets"], hb["q_lo"], hb["q_scale"], st["depth"]), rc2, st


@pytest.mark.parametrize("name", bv.MESHES)
def test_host_trees_hold_the_contract(name):
    """rt_debug_host_blas + rt_debug_check_builders over every (class, pattern) of the mesh: zero violations in the validator, every
    ACTIVE packet reached (and, by the host builder, every other packet too), rc 0 from check_builders with `reached` the number of
    triangles — the 1e30 class included, which rt_debug_check_builders refused before it compared the buffer positions exactly"""
    cases = [(cls, p) for cls in bv.CLASSES for p in bv.PATTERNS]
    parts, stats = [], []
    for cls, p in cases:
        m = bv.mesh(name, cls, p)
        part, rc, st = host_part(m)
        nt = len(m["idx"]) // 3
        assert rc == 0 and st["violations"] == 0 and st["reached"] == nt, (name, cls, p, rc, st)
        parts.append(part); stats.append((m, st))
    snap, inst_mesh = tr.link_meshes(parts)
    viol, reached = tr.validate(snap, inst_mesh)
    assert clean(viol) == {}, clean(viol)
    for k, ((cls, p), (m, st)) in enumerate(zip(cases, stats)):
        nt = len(m["bad"])
        assert reached["active"][k] == nt - m["bad"].sum() and reached["inactive"][k] == m["bad"].sum() and reached["packets"][k] == nt, (name, cls, p, reached["packets"][k])
        assert (reached["nodes"][k], reached["levels"][k]) == (st["nodes"], st["depth"]), (name, cls, p)
        fin = np.isfinite(snap["meshes"][k]["q_lo"]).all() and np.isfinite(snap["meshes"][k]["q_scale"]).all()
        assert fin and (m["bad"].any() or cls in bv.FAR), (name, cls, p)


def leaf_sorted(nodes, packets):
    """the packets with those of every leaf in the order of their primitive index"""
    out = packets.copy()
    ref = ~nodes["child"].astype(np.int64).reshape(-1)
    for r in np.unique(ref[ref >= 0]).tolist():
        first, cnt = r >> 3, (r & 7) + 1
        seg = packets[first:first + cnt]
        out[first:first + cnt] = seg[np.argsort(seg["prim"], kind="stable")]
    return out


def test_threaded_host_build_makes_the_same_tree(monkeypatch):
    """a mesh above the host builder's threading threshold (34 322 triangles: the threaded bounds, bin and partition passes), bad
    vertices in every 40th vertex and in the first third: eight threads and one thread make the same nodes, the same frame and the
    same packets in every leaf (the builder promises the SETS on either side of every split, csrc/bvh_build.cpp: within a leaf that no
    sweep ordered, the order is that of the partitions above, which are stable on several threads only), and the tree holds the
    contract"""
    for cls, p in (("nan_vertex", "every40"), ("inf_pm", "every40"), ("pinf_y", "first_third"), ("3e38_y", "first_third"), ("1e30_y", "every40")):
        m = bv.mesh("big", cls, p)
        out = {}
        for threads in ("1", "8"):
            monkeypatch.setenv("RT_BUILD_THREADS", threads)
            out[threads] = host_part(m)
        a, b = out["1"][0], out["8"][0]
        for k in (2, 4, 5):
            assert a[k].tobytes() == b[k].tobytes(), (cls, p, k)
        assert leaf_sorted(a[2], a[3]).tobytes() == leaf_sorted(b[2], b[3]).tobytes(), (cls, p)
        assert out["8"][1] == 0 and out["8"][2]["reached"] == len(m["bad"]), out["8"][1:]
        snap, inst_mesh = tr.link_meshes([b])
        viol, reached = tr.validate(snap, inst_mesh)
        assert clean(viol) == {} and reached["active"][0] == (~m["bad"]).sum(), (cls, p, clean(viol))


def test_host_builder_with_bad_vertices_is_clean_under_the_sanitizers():
    """`make sanitize-builder`: tests/native/builder_sanitize.cpp also runs build_blas + quantize_bvh2 over triangle meshes of 1, 2, 13,
    300 and 20 000 triangles with every coordinate class, on 1 and 8 threads, under AddressSanitizer and UBSan (a stand-alone host
    program: no GPU, nothing preloaded)"""
    r = subprocess.run(["make", "-C", ROOT, "sanitize-builder"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "triangle meshes, 0 failures" in r.stdout and "runtime error" not in r.stdout and "AddressSanitizer" not in r.stdout, r.stdout[-3000:]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

LIST_ROWS = np.r_[0:512, bv.N_RANDOM:bv.N_RANDOM + 512]   # the rays whose four nearest candidates the oracle restates: random and aimed ones
N_SHADE = 4096                                            # shaded rays: the first 2048 random rays and the first 2048 aimed ones, two samples of 2048 points
_REFS = {}


def shade_rays(rays):
    return np.concatenate([rays[:N_SHADE // 2], rays[bv.N_RANDOM:bv.N_RANDOM + N_SHADE // 2]])


def references(sc, key, twin=True, verts=None):
    """every reference buffer of the scene, once per key: the oracle (closest and any hits, flags and hit kinds, the four nearest
    candidates and their number, crossing counts, shaded samples and point averages, the frame) and the binary32 brute forces of the
    world-space consumers — over the twin, or (twin False: the far classes) over the vertices as they are; verts: other vertices
    (the deformed mesh of the revive case)"""
    if key in _REFS:
        return _REFS[key]
    base = sc
    if verts is not None:                                                     # mesh 0 as it is (every triangle active), mesh 2 still the twin's
        n0 = len(sc["m"]["idx"])
        base = dict(sc, verts=verts, twin_idx=np.concatenate([sc["m"]["idx"], sc["twin_idx"][n0:]]))
    orc = bv.oracle_scene(base, twin)
    rays, q = bv.rays(sc), bv.query_records(sc)
    inst = bv.instances()
    ref = {"closest": orc.intersect(rays)}
    sh = rays.copy(); sh[:, 7] = ANY_TMAX
    ref["any"] = orc.intersect(sh, any_hit=True)["inst"] >= 0
    ref["flags"], ref["kinds"] = orc.intersect_query(rays, ray_flags=api.RAY_FLAG_CULL_BACK_FACING)
    orc.tri_counts = ir.tri_counts(sc["ranges"], inst)
    ref["lists"], _, ref["list_count"] = oracle_lists(orc, rays[LIST_ROWS], None, 0, 0xFF, 4)
    ref["counts"] = ir.oracle_counts(orc, orc.tri_counts, q["points"], 3)
    s = shade_samples(orc, shade_rays(rays), N_SHADE // 2, bv.BOUNCES)
    ref["shade_s"], ref["shade_p"] = s, average_points(s, N_SHADE // 2, 2)
    ref["frame"], ref["frame_counts"] = orc.render(W, H)
    ref.update(world_brute(world_scene(base, twin), q))
    _REFS[key] = ref
    return ref


def ref_key(name, cls, pattern):
    """the cases that share their references: every bad class of a (mesh, pattern) makes the same triangles bad, but inf_pm"""
    return (name, pattern, cls if cls in bv.FAR or cls == "inf_pm" else "bad")


def run_consumers(c, sc):
    import torch
    rays = bv.rays(sc)
    got = consumers.consume(c, rays, bv.query_records(sc), ANY_TMAX, W, H)
    got["shade_s"], got["shade_p"] = (t.cpu().numpy() for t in c.shade_rays_device(consumers.dev(shade_rays(rays)), samples=2))
    torch.cuda.synchronize()
    return got


def check(got, ref, what):
    """every consumer's buffer against its reference, byte for byte"""
    n = len(ref["closest"])
    assert got["closest"].tobytes() == ref["closest"].tobytes(), (what, "closest", int(rows_differ(got["closest"], ref["closest"]).sum()))
    assert np.array_equal(got["any"], ref["any"]), (what, "any", int((got["any"] != ref["any"]).sum()))
    assert got["flags"].tobytes() == ref["flags"].tobytes(), (what, "flags")
    assert np.array_equal(got["flags_attr"][:, 7].view(np.uint32), ref["kinds"]), (what, "hit kinds")
    lists = got["hits4"].view(api.HIT_DTYPE).reshape(n, 4)
    assert lists[:, 0].tobytes() == ref["closest"].tobytes(), (what, "the nearest of the four")
    assert lists[LIST_ROWS].tobytes() == ref["lists"].tobytes() and np.array_equal(got["hits4_count"][LIST_ROWS].view(np.uint32), ref["list_count"]), (what, "hits4")
    assert np.array_equal(got["inside_count"].view(np.uint32), ref["counts"]), (what, "crossing counts")
    assert np.array_equal(got["inside"].view(np.uint32), ir.words(ref["counts"], 3, True)), (what, "vote words")
    for k in ("shade_s", "shade_p"):
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (what, k)
    for k in ("frame", "frame_plain"):
        assert got[k].view(np.uint32).tobytes() == ref["frame"].view(np.uint32).tobytes(), (what, k, int((got[k].view(np.uint32) != ref["frame"].view(np.uint32)).any(axis=2).sum()))
        assert tuple(got[k + "_counts"]) == tuple(int(x) for x in ref["frame_counts"]), (what, k)
    assert got["cp"].tobytes() == ref["cp"].tobytes(), (what, "closest points", int(rows_differ(got["cp"], ref["cp"]).sum()))
    assert got["sweep"].tobytes() == ref["sweep"].tobytes(), (what, "sweeps", int(rows_differ(got["sweep"], ref["sweep"]).sum()))
    for k in ("boxes", "tris"):
        rc_, ri = ref[k]
        assert got[k + "_count"].astype(rc_.dtype).tobytes() == rc_.tobytes(), (what, k)
        assert got[k + "_ids"].astype(ri.dtype).tobytes() == np.ascontiguousarray(ri[:, :16]).tobytes(), (what, k)
    consumers.check_signed_distance(got, what)


def validate(c, sc, what, active=None):
    """the snapshot passes the validator; every active packet is reached"""
    snap = c.debug_snapshot()
    viol, reached = tr.validate(snap, bv.INST_MESH)
    assert clean(viol) == {}, (what, clean(viol))
    nt = len(sc["m"]["bad"])
    want = int((~sc["m"]["bad"]).sum()) if active is None else active
    assert reached["active"] == {0: want, 1: 12, 2: 0} and reached["inactive"][0] == nt - want, (what, reached["active"], reached["inactive"])
    return snap


def clean_verts(sc):
    v = sc["verts"].copy()
    v[:sc["ranges"][1][0]].reshape(-1, 6)[sc["m"]["idx"].astype(np.int64), :3] = sc["m"]["clean"].reshape(-1, 3)
    return v


def span_of(sc):
    return 6 * (int(sc["m"]["idx"].max()) + 1)


def deformed_verts(sc):
    """the scene's vertices with mesh 0 at its clean positions, displaced by a sine field: all finite over the mesh's span"""
    v = clean_verts(sc)
    p = v[:span_of(sc)].reshape(-1, 6)[:, :3]
    p += (np.float32(0.15) * np.sin(np.float32(2.5) * p[:, [1, 2, 0]] + np.float32(0.7))).astype(np.float32)
    return v


def setup(c, sc, verts=None):
    c.upload_geometry(sc["verts"] if verts is None else verts, sc["idx"], sc["ranges"])   # RT_OK from rt_upload_geometry and every rt_build_blas, or RtError
    c.set_uniforms(sc["uniforms"])
    c.set_skybox(bv.scenes.synthetic_skybox(64))
    c.set_instances(bv.instances())                                                       # RT_OK over the all-bad mesh 2 as well


def run_producer(producer, name, cls, pattern, mp):
    import torch
    sc = bv.scene(name, cls, pattern)
    what = "%s, %s, %s, %s" % (producer, name, cls, pattern)
    far = cls in bv.FAR
    c = RtContext(0)
    try:
        kind, _, builder = producer.partition("_")
        builder = builder or kind
        use_builder(c, builder, mp)
        key, verts, active = ref_key(name, cls, pattern), None, None
        if kind == "refit":
            # the bad vertices reach the device through a refit only: rejected for a position that is not finite (the statuses of
            # rt_refit_blas_device are unchanged), taken otherwise; rt_build_blas then builds over what the device holds
            setup(c, sc, clean_verts(sc))
            t = torch.from_numpy(sc["verts"][:span_of(sc)].reshape(-1, 6).copy()).to("cuda:0")
            torch.cuda.synchronize()
            if cls in bv.NON_FINITE:
                with pytest.raises(RtError) as e:
                    c.refit_blas_device(0, t)
                assert e.value.code == RT_ERR_INVALID_ARGUMENT and "not finite" in str(e.value), what
            else:
                c.refit_blas_device(0, t)
            c.build_blas(0)
            c.set_instances(bv.instances())
        else:
            setup(c, sc)
        if kind == "revive":
            validate(c, sc, what + " (before the refit)")
            verts = deformed_verts(sc)
            t = torch.from_numpy(verts[:span_of(sc)].reshape(-1, 6).copy()).to("cuda:0")
            torch.cuda.synchronize()
            c.refit_blas_device(0, t)
            c.set_instances(bv.instances())
            key, active = ref_key(name, cls, pattern) + ("revived",), len(sc["m"]["bad"])                     # every triangle of mesh 0 is active again
        got = run_consumers(c, sc)
        snap = validate(c, sc, what, active)
        if builder != "host" and kind != "revive":
            c.build_blas(0)                                                                   # the device builders are deterministic
            c.set_instances(bv.instances())
            again = c.debug_snapshot()
            for k in ("blas_nodes", "packets", "meshes", "cover_boxes"):
                assert again[k].tobytes() == snap[k].tobytes(), (what, k)
        check(got, references(sc, key, twin=not far or kind == "revive", verts=verts), what)   # (the far classes: the vertices as they are)
    finally:
        c.close()


PRODUCERS = ["host", "1", "2", "3", "refit_host", "refit_3", "revive_host", "revive_3"]


@pytest.mark.gpu
@pytest.mark.parametrize("cls", list(bv.CLASSES))
@pytest.mark.parametrize("producer", PRODUCERS)
def test_a_bad_vertex_costs_the_mesh_nothing(producer, cls, monkeypatch):
    """the teapot with the class in every 40th vertex, under every producer of a BLAS, all consumers against the references"""
    run_producer(producer, "teapot", cls, "every40", monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("name,pattern", OTHER_CASES)
@pytest.mark.parametrize("builder", ["host", "3"])
def test_other_patterns_and_meshes(builder, name, pattern, monkeypatch):
    for cls in OTHER_CLASSES.get(name, SMALL_CLASSES):
        run_producer(builder, name, cls, pattern, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "3"])
def test_the_all_bad_instance_costs_the_scene_nothing(builder, monkeypatch):
    """every buffer of the scene equals that of a scene that lacks the instance of the all-bad mesh (the last record), the cube's
    answers among them; rt_set_instances over the all-bad mesh is RT_OK"""
    sc = bv.scene("teapot", "nan_vertex", "every40")
    c = RtContext(0)
    try:
        use_builder(c, builder, monkeypatch)
        setup(c, sc)
        got = run_consumers(c, sc)
        ref = references(sc, ref_key("teapot", "nan_vertex", "every40"))
        assert (ref["closest"]["inst"] == 2).sum() >= 100 and not (ref["closest"]["inst"] == 3).any()
        c.set_instances(bv.instances(3))
        consumers.assert_same(got, run_consumers(c, sc), consumers.RAY_CONSUMERS + consumers.WORLD_CONSUMERS, builder, "the scene's without the all-bad instance")
    finally:
        c.close()
