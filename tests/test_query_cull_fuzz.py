"""The conservative culls of the record-level queries against their brute-force references, on the seeded adversarial scenes and
records of tests/query_cull_cases.py (run with `-m gpu` on a real MI355X).  rt_api.h says of every one of these queries that its answer
"depends on the record, the instance record and the packet only, never on the tree": for every scene and query, every output of the
device form equals the tree-free binary32 restatement of that query's own reference module byte for byte, under three cull masks, in
every pruning variant of the list forms, and under every tree producer (the device builder, blas_builder 0, RT_GPU_BVH_ALGO 1 and 2,
device instance records, a TLAS update after every instance moved, a refitted BLAS of the large mesh), and once more with each
anisotropic, sheared or cancelling instance of the large mesh alone in the scene, where the walks prune inside it.  The last test proves from the
counting host forms that the culls were engaged, family by family.  One test is one scene and one query.

The two list forms of the ray query ride on the point records: rt_point_inside_device's counts against the oracle and against the
count-only rt_intersect_device_hits composed from the same rays, and rt_intersect_device_hits at max_hits 4 with counts and attributes
against the oracle's sorted candidate lists (tests/test_ray_query_hits.py's check)."""
import numpy as np
import pytest

from tests import inside_reference as ir
from tests import query_cull_cases as qc
from tests import test_closest_point as tcp
from tests import test_closest_point_hits as tch
from tests import test_closest_segment as tcs
from tests import test_closest_triangle as tct
from tests import test_overlap_boxes as tob
from tests import test_point_inside as tpi
from tests import test_ray_query_hits as trh
from tests import test_sphere_sweep as tss
from tests import test_triangle_overlaps as tto
from tests.test_ray_query import dev_inst
from tests.test_ray_query_oracle import oracle_scene, use_builder
from vulkan_raytracing_amd import RtContext

pytestmark = pytest.mark.gpu
SEED = qc.DEFAULT_SEED
ALGO_SCENES = (1, 6)          # RT_GPU_BVH_ALGO 1 and 2 on these two
REFIT_SCENE = 0
ATTRIBUTE_STRIDE = {"closest_point": 1, "closest_segment": 8, "closest_triangle": 16}   # (the imported checks compute their own brute force)

# Engagement conditions a family does not have to meet, with the reason: (query form, instance family or "*", record family or "*").
# test_the_query_culls_were_engaged lists what it skips and flags an entry that prunes after all.
_EVERY_CANDIDATE = "the count is of every candidate within r_max, and these records have r_max = inf: every triangle is one"
NOT_ENGAGED = {(form, "*", f): _EVERY_CANDIDATE for form in ("closest_point_hits, 4 rows with counts", "closest_point_hits, counts alone")
               for f in qc.POINT_FAMILIES}


# The same for the large instances alone in their scene: (query form, scene, instance) -> the reason.  The slack that a walk subtracts
# from every box distance inside an instance is 2^-16 (the overlaps: 2^-13) of the largest magnitude in play, divided by s_i.
_OBJECT_MAGNITUDE = ("the mesh lies 1000 to 10 000 from the object-space origin: the slack, that share of this magnitude over s_i, exceeds the "
                     "mesh's own extent, so no box of it is ever far enough")
_WORLD_MAGNITUDE = "the scene lies 1e3 (scene 5) or 1e5 (scene 7) from the origin: the slack, that share of this magnitude over s_i, exceeds the mesh's extent"
_SLACK_FORMS = ("closest_point", "closest_point_hits, 4 rows pruned", "overlap_triangles, 4 ids with counts", "sweep_spheres", "closest_segment",
                "closest_triangle")
ALONE_NOT_ENGAGED = {(form, "scene00", 2): _OBJECT_MAGNITUDE for form in _SLACK_FORMS + ("overlap_boxes, 4 ids with counts",)}
ALONE_NOT_ENGAGED.update({(form, "scene04", 0): _OBJECT_MAGNITUDE for form in ("overlap_boxes, 4 ids with counts", "overlap_triangles, 4 ids with counts")})
ALONE_NOT_ENGAGED.update({(form, "scene05", 1): _WORLD_MAGNITUDE for form in _SLACK_FORMS})
ALONE_NOT_ENGAGED.update({(form, "scene07", 2): _WORLD_MAGNITUDE for form in _SLACK_FORMS + ("overlap_boxes, 4 ids with counts",)})


class _Failures:
    def __init__(self, w, query):
        self.w, self.query, self.lines = w, query, []

    def rows(self, config, name, got, want, recs, fam):
        """byte comparison per record of one output array"""
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        n = len(recs)
        if got.shape != want.shape or got.dtype.itemsize != want.dtype.itemsize:
            self.lines.append("seed %d, %s, %s, [%s] %s: shape %s %s against %s %s" % (SEED, self.w.scene.name, self.query, config, name, got.shape, got.dtype, want.shape, want.dtype))
            return
        if got.tobytes() == want.tobytes():
            return
        g, r = got.view(np.uint8).reshape(n, -1), want.view(np.uint8).reshape(n, -1)
        bad = np.nonzero((g != r).any(axis=1))[0]
        i = int(bad[0])
        per = {f: int((fam[bad] == f).sum()) for f in np.unique(fam[bad])}
        self.lines.append("seed %d, %s, %s, [%s] %s: %d of %d records differ %s; first: family %s, record %d = %s (hex %s), device %s (hex %s), reference %s (hex %s)"
                          % (SEED, self.w.scene.name, self.query, config, name, len(bad), n, per, fam[i], i, recs[i].tolist(), recs[i].tobytes().hex(),
                             got[i].tolist(), got[i].tobytes().hex(), want[i].tolist(), want[i].tobytes().hex()))

    def helper(self, config, fn, *args, **kw):
        """one of the imported checks of the query's own test file"""
        try:
            return fn(*args, **kw)
        except AssertionError as e:
            self.lines.append("seed %d, %s, %s, [%s] %s.%s: %s" % (SEED, self.w.scene.name, self.query, config, fn.__module__, fn.__name__, str(e)[:1500]))


def _device(c, w, query, recs, fam, cull, ref, fails, config, full):
    """every device form of the query at one cull mask against the reference; full: the list forms in all their pruning variants"""
    if query == "closest_point":
        h, _ = tcp.gpu_closest(c, recs, cull, attributes=False)
        fails.rows(config, "hits", h, ref, recs, fam)
    elif query == "closest_point_hits":
        for K in (1, 4, 16) if full else (4,):
            h, _, cnt = tch.gpu_k(c, recs, K, cull)
            fails.rows(config, "rows, max_hits %d with counts" % K, h, ref[0][:, :K], recs, fam)
            fails.rows(config, "counts, max_hits %d" % K, cnt, ref[1], recs, fam)
            h, _, cnt = tch.gpu_k(c, recs, K, cull, counts=False)
            fails.rows(config, "rows, max_hits %d pruned" % K, h, ref[0][:, :K], recs, fam)
        if full:
            _, _, cnt = tch.gpu_k(c, recs, 0, cull)
            fails.rows(config, "counts alone", cnt, ref[1], recs, fam)
    elif query in ("overlap_boxes", "overlap_triangles"):
        mod = tob if query == "overlap_boxes" else tto
        z = fam == "degenerate" if query == "overlap_triangles" else np.zeros(len(recs), bool)

        def both(**kw):
            """the zero-area query triangles run with the singular instances left out (rt_api.h leaves such pairs open)"""
            cnt, ids = mod.gpu_overlap(c, recs, cull=cull, **kw)
            if z.any():
                c2, i2 = mod.gpu_overlap(c, recs[z], cull=w.overlap_cull(cull), **kw)
                if cnt is not None:
                    cnt[z] = c2
                if ids is not None:
                    ids[z] = i2
            return cnt, ids

        for K in (4, 16) if full else (16,):
            cnt, ids = both(max_ids=K)
            fails.rows(config, "counts, max_ids %d" % K, cnt, ref[0], recs, fam)
            fails.rows(config, "ids, max_ids %d with counts" % K, ids, ref[1][:, :K], recs, fam)
            cnt, ids = both(max_ids=K, counts=False)
            fails.rows(config, "ids, max_ids %d pruned" % K, ids, ref[1][:, :K], recs, fam)
        occ, _ = both(max_ids=0, any=True)
        fails.rows(config, "RT_OVERLAP_ANY", occ, (ref[0] > 0).astype(np.uint32), recs, fam)
    elif query == "sweep_spheres":
        h, _ = tss.gpu_sweep(c, recs, cull)
        fails.rows(config, "hits", h, ref, recs, fam)
    elif query == "closest_segment":
        h, _, s = tcs.gpu_segments(c, recs, cull, attributes=False)
        fails.rows(config, "hits", h, ref[0], recs, fam)
        fails.rows(config, "d_params", s, ref[1], recs, fam)
    elif query == "closest_triangle":
        h, _, quv = tct.gpu_triangles(c, recs, cull, attributes=False)
        fails.rows(config, "hits", h, ref[0], recs, fam)
        fails.rows(config, "d_params", quv, ref[1], recs, fam)
    else:
        raise ValueError(query)


def _attributes(c, w, orc, query, recs, fam, fails):
    """the imported checks of the queries' own files: attributes against the oracle's hit_attributes, side words, the n == 0 forms"""
    S = w.S
    if query in ATTRIBUTE_STRIDE:
        sub = recs[::ATTRIBUTE_STRIDE[query]]
        if query == "closest_point":
            fails.helper("attributes", tcp.check, S, orc, sub, tcp.gpu_closest(c, sub), what="fuzz")
        elif query == "closest_segment":
            fails.helper("attributes", tcs.check, S, orc, sub, tcs.gpu_segments(c, sub), what="fuzz")
        else:
            fails.helper("attributes", tct.check, S, orc, sub, tct.gpu_triangles(c, sub), what="fuzz")
    elif query == "sweep_spheres":
        fails.helper("hits", tss.check, tss.gpu_sweep(c, recs)[0], w.reference(query, 0xFF), recs, "fuzz")
    elif query == "closest_point_hits":
        ref = w.reference(query, 0xFF)
        fails.helper("rows", tch.check_both_walks, c, recs, ref, 4, what="fuzz")
    elif query in ("overlap_boxes", "overlap_triangles"):
        mod = tob if query == "overlap_boxes" else tto
        keep = fam != "degenerate"
        ref = w.reference(query, 0xFF)
        fails.helper("rows", mod.check, mod.gpu_overlap(c, recs[keep]), (ref[0][keep], ref[1][keep]), "fuzz")


def _inside(c, w, orc, recs, fam, culls, fails, config):
    """rt_point_inside_device's counts against the oracle and against the composed rt_intersect_device_hits count-only query, its words
    against the restated vote (tests/test_point_inside.py's check); rt_signed_distance_device: rt_closest_point_device's reference with
    bit 0 of the word as the sign of t"""
    import torch
    tc = ir.tri_counts(w.scene.ranges, w.scene.instances)
    for cull in culls:
        counts = w.cached(("inside", cull), lambda: ir.oracle_counts(orc, tc, recs, 3, cull))
        valid = np.isfinite(recs[:, :3]).all(axis=1)
        out = fails.helper(config + ", cull %#x" % cull, tpi.check, c, recs[valid], 3, counts[valid], "fuzz", cull)
        rays = ir.compose_rays(recs[valid], 3)
        orc.tri_counts = tc
        lists = w.cached(("ray lists", cull), lambda: trh.oracle_lists(orc, rays, None, 0, cull, 4))
        fails.helper(config + ", cull %#x, rt_intersect_device_hits max_hits 4" % cull, trh.check_lists, orc,
                     trh.gpu_hits(c, rays, None, 0, cull, 4, attributes=True), lists, "fuzz")
        if out is None:
            continue
        words = np.zeros(len(recs), np.uint32); words[valid] = out[0]
        res = c.signed_distance_device(tpi.dev(recs), n_dirs=3, cull_mask=cull)
        torch.cuda.synchronize()
        sh, _ = res.numpy()
        want = w.reference("point_inside", cull).copy()
        ok = valid & (recs[:, 3] >= 0)
        raw = want.view(np.uint32).reshape(len(want), 5)
        raw[ok, 0] |= (words[ok] & 1) << 31
        fails.rows(config + ", cull %#x" % cull, "the signed t", sh, want, recs, fam)


def _engagement(c, w, query, recs, fam, tgt, fails):
    """[(form, instance family, record family, records, triangle tests, node visits, admitted triangles, instance or -1, alone)] from
    the counting host forms, one call per record family and target instance.  The anisotropic, sheared and cancelling instances of the
    large mesh run once more alone in the scene, where their boxes prune: there every device form of the query is also held to the
    brute force over that one instance, byte for byte (`fails`)"""
    sc = w.scene
    adm = w.admitted_triangles(0xFF)
    forms = {"closest_point": [("closest_point", lambda r: c.closest_point(r, counting=True)[-1])],
             "closest_point_hits": [("closest_point_hits, 4 rows pruned", lambda r: c.closest_point_hits(r, 4, counts=False, counting=True)[-1]),
                                    ("closest_point_hits, 4 rows with counts", lambda r: c.closest_point_hits(r, 4, counting=True)[-1]),
                                    ("closest_point_hits, counts alone", lambda r: c.closest_point_hits(r, 0, counting=True)[-1])],
             "point_inside": [("point_inside", lambda r: c.point_inside(r, counting=True)[-1])],
             "overlap_boxes": [("overlap_boxes, 4 ids with counts", lambda r: c.overlap_boxes(r, 4, counting=True)[-1]),
                               ("overlap_boxes, any", lambda r: c.overlap_boxes(r, 0, any=True, counting=True)[-1])],
             "overlap_triangles": [("overlap_triangles, 4 ids with counts", lambda r: c.overlap_triangles(r, 4, counting=True)[-1]),
                                   ("overlap_triangles, any", lambda r: c.overlap_triangles(r, 0, any=True, counting=True)[-1])],
             "sweep_spheres": [("sweep_spheres", lambda r: c.sweep_spheres(r, counting=True)[-1])],
             "closest_segment": [("closest_segment", lambda r: c.closest_segment(r, counting=True)[-1])],
             "closest_triangle": [("closest_triangle", lambda r: c.closest_triangle(r, counting=True)[-1])]}[query]
    rows = []
    for f in np.unique(fam):
        if f == "invalid":
            continue
        for t in np.unique(tgt[fam == f]):
            sub = recs[(fam == f) & (tgt == t)]
            ifam = sc.families[t][0] if t >= 0 else "any"
            for form, call in forms:
                st = call(sub)
                rows.append((form, ifam, str(f), len(sub), int(st.tri_tests), int(st.node_visits), adm, int(t), False))
    # the anisotropic, sheared and cancelling instances of the large mesh once more, each alone in the scene: the world-space slack
    # of a walk takes in the largest row-term magnitude of ANY instance (word 0 of the scale array), so a cancelling or huge
    # neighbour widens it for all; alone, what remains is the instance's own
    for t in np.unique(tgt[tgt >= 0]):
        if sc.families[t][0] in ("anisotropic", "sheared", "cancelling") and sc.mesh_of(t) in qc.LARGE_MESHES:
            c.set_instances(sc.instances[[t]])
            w1 = w.alone(t)
            w1.use_records(query, recs[tgt == t], fam[tgt == t])
            if query == "point_inside":
                _inside(c, w1, oracle_scene(*w1.scene.parts), recs[tgt == t], fam[tgt == t], (0xFF,), fails, "instance %d alone" % t)
            else:
                _device(c, w1, query, recs[tgt == t], fam[tgt == t], 0xFF, w1.reference(query, 0xFF), fails, "instance %d alone, cull 0xff" % t, True)
            for f in np.unique(fam[tgt == t]):
                sub = recs[(fam == f) & (tgt == t)]
                for form, call in forms:
                    st = call(sub)
                    rows.append((form, sc.families[t][0], str(f), len(sub), int(st.tri_tests), int(st.node_visits), int(w.n_tris[t]), int(t), True))
    c.set_instances(sc.instances)
    return rows


def _run(c, c_host, index, query):
    import torch
    w = qc.world(index, SEED)
    sc = w.scene
    recs, fam, tgt = w.records(query)
    fails = _Failures(w, query)
    orc = oracle_scene(*sc.parts)
    culls = w.culls(query)
    rng = np.random.default_rng([SEED, index, 9])
    moved = sc.instances.copy()
    moved["transform"][:, [3, 7, 11]] += rng.uniform(-0.5, 0.5, (len(moved), 3)).astype(np.float32)

    def everything(ctx, config, full):
        for cull in culls if full else culls[:1]:
            if query == "point_inside":
                _inside(ctx, w, orc, recs, fam, (cull,), fails, config)
            else:
                step = qc.CULL_STRIDE.get(query, 1) if cull != 0xFF else 1
                _device(ctx, w, query, recs[::step], fam[::step], cull, w.reference(query, cull, step), fails, "%s, cull %#x" % (config, cull), full)

    c.upload_geometry(sc.verts, sc.idx, sc.ranges)
    c.set_instances(sc.instances)
    everything(c, "device builder, host records", True)
    if query != "point_inside":
        _attributes(c, w, orc, query, recs, fam, fails)
    rows = _engagement(c, w, query, recs, fam, tgt, fails)
    torch.cuda.synchronize()
    c.set_instances_device(dev_inst(sc.instances))
    everything(c, "device builder, rt_set_instances_device", False)
    c.set_instances(moved)
    c.set_instances(sc.instances, update=True)
    everything(c, "device builder, every instance moved and a TLAS update back", False)
    torch.cuda.synchronize()
    c.set_instances_device(dev_inst(moved))
    c.set_instances_device(dev_inst(sc.instances), update=True)
    everything(c, "device builder, device records moved and a TLAS update back", False)
    c_host.upload_geometry(sc.verts, sc.idx, sc.ranges)
    c_host.set_instances(sc.instances)
    everything(c_host, "blas_builder 0", False)
    if index in ALGO_SCENES:
        for algo in ("1", "2"):
            with pytest.MonkeyPatch.context() as mp:
                ca = RtContext(0)
                try:
                    use_builder(ca, algo, mp)
                    ca.upload_geometry(sc.verts, sc.idx, sc.ranges)
                    ca.set_instances(sc.instances)
                    everything(ca, "RT_GPU_BVH_ALGO %s" % algo, False)
                finally:
                    ca.close()
    return fails, rows


@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_host_trees():
    c = RtContext(0)
    c.set_param("blas_builder", 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def results(ctx, ctx_host_trees):
    """(scene index, query) -> (failures, engagement rows), run once"""
    done = {}

    def get(index, query):
        if (index, query) not in done:
            try:
                done[(index, query)] = _run(ctx, ctx_host_trees, index, query)
            except AssertionError:
                raise
            except Exception as e:       # an error of the library (a GPU fault among them): nothing more is started on the GPU
                pytest.exit("scene %d, %s (seed %d): %s: %s" % (index, query, SEED, type(e).__name__, e), returncode=3)
        return done[(index, query)]

    return get


@pytest.mark.parametrize("query", qc.QUERIES)
@pytest.mark.parametrize("index", range(qc.N_SCENES))
def test_no_tree_changes_an_answer(results, index, query):
    """every output of the query on the scene equals its brute-force reference byte for byte: three cull masks and every pruning
    variant on the device builder's trees; rt_set_instances_device records, TLAS updates from moved records (host and device),
    blas_builder 0 and (scenes 1 and 6) RT_GPU_BVH_ALGO 1 and 2 at cull mask 0xFF.  Wall time on an MI355X machine, the references
    computed in the test: closest_triangle 7.4 to 8.7 s, closest_segment 3.1 s, every other query under 3 s, the file 150 s; with
    the references already in the process's cache (tests/test_query_cull_cases.py ran before) 0.1 to 0.85 s per test and 29 s for
    the file."""
    fails, rows = results(index, query)
    assert len(rows) > 0
    assert not fails.lines, "%d differences\n%s" % (len(fails.lines), "\n".join(fails.lines[:8]))


def test_a_refitted_blas_of_the_large_mesh(ctx):
    """rt_refit_blas_device of the large mesh with perturbed vertices, rt_set_instances_device, and every query against the reference
    rebuilt over the new vertices (closest_triangle and closest_segment on every fourth record)"""
    import types

    import torch
    from tests.test_blas_refit import deform, with_mesh
    w = qc.world(REFIT_SCENE, SEED)
    sc = w.scene
    geom = types.SimpleNamespace(verts=sc.verts, idx=sc.idx, ranges=sc.ranges)
    try:
        ctx.upload_geometry(sc.verts, sc.idx, sc.ranges)
        ctx.set_instances(sc.instances)
        t = deform(geom, qc.LARGE, amp=0.05)
        torch.cuda.synchronize()
        ctx.refit_blas_device(qc.LARGE, t)
        torch.cuda.synchronize()
        ctx.set_instances_device(dev_inst(sc.instances))
        v2 = with_mesh(geom, sc.verts, qc.LARGE, t)
    except AssertionError:
        raise
    except Exception as e:
        pytest.exit("refit of scene %d (seed %d): %s: %s" % (REFIT_SCENE, SEED, type(e).__name__, e), returncode=3)
    sc2 = qc.Scene(sc.index, sc.seed, v2, sc.idx, sc.ranges, sc.instances, sc.families, sc.meta, sc.shift)
    w2 = qc.World(sc2, SEED)
    lines = []
    for query in qc.QUERIES:
        if query == "point_inside":
            continue
        recs, fam, _ = w.records(query)
        step = 4 if query in ("closest_segment", "closest_triangle") else 1
        recs, fam = recs[::step], fam[::step]
        w2.use_records(query, recs, fam)
        fails = _Failures(w2, query)
        try:
            _device(ctx, w2, query, recs, fam, 0xFF, w2.reference(query, 0xFF), fails, "refitted large mesh", False)
        except AssertionError:
            raise
        except Exception as e:
            pytest.exit("refit of scene %d, %s (seed %d): %s: %s" % (REFIT_SCENE, query, SEED, type(e).__name__, e), returncode=3)
        lines += fails.lines
    assert not lines, "%d differences\n%s" % (len(lines), "\n".join(lines[:8]))


def _exempt(form, ifam, f):
    for key in ((form, ifam, f), (form, "*", f), (form, ifam, "*"), (form, "*", "*")):
        if key in NOT_ENGAGED:
            return key
    return None


def test_the_query_culls_were_engaged(results):
    """Without this the module could pass with every cull switched off.  From the counting host forms at cull mask 0xFF, per (query
    form, family of the instance the records were placed against, record family), summed over the scenes: the triangle tests are
    strictly fewer than records x admitted triangles; and for every anisotropic, sheared or cancelling instance of the large mesh, the
    triangle tests of the records placed against it are fewer than records x 640, that mesh's triangles alone: the walk prunes inside
    the instance, measured with the instance alone in the scene (see _engagement).  An entry of NOT_ENGAGED that prunes after all is
    an error too.  Measured on an MI355X at the default seed, triangle tests over records x admitted triangles, by the family of the
    instance the records were placed against (any: volume, far, equidistant, spanning and radius_at_answer records):

    form                                      anisotropic          any   cancelling   coincident         huge       nested rigid_dyadic      sheared         tiny
    closest_point                                   0.229        0.177        0.311        0.140        0.503        0.158        0.167        0.270        0.097
    closest_point_hits, 4 rows pruned               0.231        0.182        0.312        0.152        0.504        0.162        0.184        0.272        0.100
    closest_point_hits, 4 rows with counts          1.000        0.476        1.000        1.000        1.000        1.000        1.000        1.000        1.000
    closest_point_hits, counts alone                1.000        0.476        1.000        1.000        1.000        1.000        1.000        1.000        1.000
    closest_segment                                 0.233        0.142        0.338        0.149        0.503        0.187        0.182        0.278        0.124
    closest_triangle                                0.252        0.172        0.347        0.184        0.512        0.218        0.219        0.293        0.153
    overlap_boxes, 4 ids with counts                0.233            -        0.436        0.300        0.502        0.272        0.362        0.274        0.409
    overlap_boxes, any                              0.118            -        0.322        0.119        0.333        0.208        0.257        0.203        0.264
    overlap_triangles, 4 ids with counts            0.302            -        0.523        0.444        0.561        0.358        0.422        0.366        0.478
    overlap_triangles, any                          0.110            -        0.352        0.146        0.394        0.212        0.228        0.232        0.270
    point_inside                                    0.003        0.002        0.003        0.007        0.005        0.005        0.004        0.003        0.003
    sweep_spheres                                   0.237            -        0.281        0.111        0.476        0.072        0.145        0.255        0.092

    and by record family (every instance family together):

    closest_point                           box_corner 0.239  near_surface 0.211  on_feature 0.206  equidistant 0.218  far 0.275  radius_at_answer 0.127  volume 0.266
    closest_point_hits, 4 rows pruned       box_corner 0.243  near_surface 0.220  on_feature 0.213  equidistant 0.234  far 0.291  radius_at_answer 0.127  volume 0.274
    closest_point_hits, with counts / alone every family 1.000 (NOT_ENGAGED), radius_at_answer 0.127
    closest_segment                         crossing 0.221  nearly_parallel 0.212  point 0.210  spanning 0.305  tiny 0.211  radius_at_answer 0.142
    closest_triangle                        crossing 0.232  degenerate 0.213  nearly_parallel 0.216  spanning 0.405  tiny 0.215  radius_at_answer 0.172
    overlap_boxes, 4 ids with counts        box_corner 0.313  collapsed 0.314  tiny_and_enclosing 0.308  volume 0.330  coplanar_face 0.383
    overlap_boxes, any                      box_corner 0.288  collapsed 0.187  tiny_and_enclosing 0.127  volume 0.204  coplanar_face 0.268
    overlap_triangles, 4 ids with counts    crossing 0.369  degenerate 0.319  nearly_parallel 0.328  spanning 0.723  tiny 0.301
    overlap_triangles, any                  crossing 0.179  degenerate 0.211  nearly_parallel 0.228  spanning 0.224  tiny 0.222
    point_inside                            box_corner 0.002  near_surface 0.004  on_feature 0.007  equidistant 0.005  far 0.001  volume 0.001
    sweep_spheres                           aimed 0.170  axis_parallel 0.144  grazing 0.167  inside 0.197  radii 0.373  scaled_d 0.168  tmax 0.155

    Inside the scene, every record placed against an anisotropic, sheared or cancelling instance of the large mesh tests all of its
    640 triangles: the world-space slack of a walk takes in the largest row-term magnitude of any instance (word 0 of the scale
    array) and is divided by s_i on entry, so one cancelling or huge neighbour, or a scene 1000 and more from the origin, opens
    every box of an instance whose s_i is small.  That is the price of the conservative slack, not an error.  So each such instance
    runs once more alone in its scene (_engagement): there every output is again held to the brute force byte for byte, and the
    condition is asserted per form and instance (the instance's record families together; the counting forms of the K nearest query
    left out; ALONE_NOT_ENGAGED names the pairs at 1.0000 with the reason).  Triangle tests over records x 640 (scene:instance,
    family; 00:0 condition 500, 00:2 100, 02:2 1000, 04:0 10, 05:1 100 and 1e3 out, 07:2 10 and 1e5 out, the shears 1e-3):

    form                                   00:0 aniso 00:2 cance 01:0 shear 02:2 aniso 04:0 cance 04:1 shear 05:1 aniso 07:2 aniso
    closest_point                              0.3723     1.0000     0.4324     0.3947     0.9941     0.4484     1.0000     1.0000
    closest_point_hits, 4 rows pruned          0.4163     1.0000     0.8460     0.9439     0.9979     0.8536     1.0000     1.0000
    closest_segment                            0.3235     1.0000     0.3843     0.3773     0.9972     0.3505     1.0000     1.0000
    closest_triangle                           0.2460     1.0000     0.5407     0.5914     0.9965     0.5391     1.0000     1.0000
    overlap_boxes, 4 ids with counts           0.4537     1.0000     0.6690     0.5767     1.0000     0.6557     0.9773     1.0000
    overlap_boxes, any                         0.1793     0.6472     0.2830     0.2977     0.5755     0.3019     0.4657     0.5071
    overlap_triangles, 4 ids with counts       0.6763     1.0000     0.8326     0.8555     1.0000     0.7956     1.0000     1.0000
    overlap_triangles, any                     0.3811     0.6619     0.4505     0.3695     0.5427     0.3904     0.5062     0.5157
    point_inside                               0.0088     0.0145     0.0084     0.0060     0.0123     0.0096     0.0122     0.0115
    sweep_spheres                              0.9588     1.0000     0.9942     0.9935     0.9921     0.9906     1.0000     1.0000

    The sweep prunes least: sweep_box inflates every box by the reach of the sphere over the box's own diagonal, divided by s_i.
    """
    fam, large = {}, []
    for index in range(qc.N_SCENES):
        sc = qc.world(index, SEED).scene
        for query in qc.QUERIES:
            for form, ifam, f, n, tests, visits, adm, t, alone in results(index, query)[1]:
                if alone:
                    large.append((form, sc.name, t, ifam, f, n, tests, n * adm))
                    continue
                e = fam.setdefault((form, ifam, f), [0, 0, 0, 0])
                e[0] += n; e[1] += tests; e[2] += visits; e[3] += n * adm
    print("engagement (seed %d): form | instance family | record family | records | triangle tests / (records x admitted) | node visits per record" % SEED)
    missed = []
    for (form, ifam, f), (n, tests, visits, bound) in sorted(fam.items()):
        print("%-40s %-13s %-20s %6d  %.4f  %8.1f" % (form, ifam, f, n, tests / bound, visits / n))
        key = _exempt(form, ifam, f)
        if key is not None:
            if tests < bound:
                missed.append("%s / %s / %s is listed in NOT_ENGAGED %s and prunes after all (%d of %d): take it off the list" % (form, ifam, f, key, tests, bound))
        elif not 0 < tests < bound:
            missed.append("%s / %s / %s: %d triangle tests, records x admitted triangles %d" % (form, ifam, f, tests, bound))
    print("inside the anisotropic, sheared and cancelling instances of the large mesh, each alone: form | scene | instance | family | record family | tests / (records x 640)")
    inside = {}
    for form, name, t, ifam, f, n, tests, bound in large:
        print("%-40s %s %d %-12s %-20s %.4f" % (form, name, t, ifam, f, tests / bound))
        if _exempt(form, ifam, f) is None:
            e = inside.setdefault((form, name, t, ifam), [0, 0])
            e[0] += tests; e[1] += bound
    print("per form and instance, its record families together: form | scene | instance | family | tests / (records x 640)")
    for (form, name, t, ifam), (tests, bound) in sorted(inside.items()):
        print("%-40s %s %d %-12s %.4f" % (form, name, t, ifam, tests / bound))
        if (form, name, t) in ALONE_NOT_ENGAGED:
            if tests < bound:
                missed.append("%s, %s instance %d is listed in ALONE_NOT_ENGAGED and prunes after all (%d of %d): take it off the list" % (form, name, t, tests, bound))
        elif not tests < bound:
            missed.append("%s, %s instance %d (%s) alone: %d triangle tests, records x 640 = %d: no pruning inside the instance" % (form, name, t, ifam, tests, bound))
    assert len(large) > 0
    assert not missed, "\n".join(missed)
