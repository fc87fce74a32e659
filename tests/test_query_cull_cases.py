"""The inputs of tests/test_query_cull_fuzz.py, checked without a GPU (tests/query_cull_cases.py): the generator is deterministic, every
instance is what its family says (binary64 predicates over the binary32 records), the aspect floor holds, and the brute-force
references alone can referee the records: enough of every record family hits something, the equidistant points tie, the radii at the
answer give hits and misses, coincident answers name the smaller instance, and every query's binary32 restatement is held to its
binary64 sibling by the criterion of that query's own test file under condition numbers of up to 1000 (MEASURED_WORST and MEASURED:
where it is not met, twice the measured figure).

CPU time of the references on the development host, per scene at cull mask 0xFF: closest_point 2.6 s, closest_point_hits 2 s,
overlap_boxes 0.1 s, overlap_triangles 0.6 s, sweep_spheres 0.6 to 4.7 s, closest_segment 8 s, closest_triangle 23 s (about 10 us
per pair); the closest-triangle conditions are therefore checked on TRIANGLE_SCENES only.  The references are cached per process
(query_cull_cases.world), so the GPU file does not compute them again when the whole suite runs."""
import numpy as np
import pytest

from tests import closest_reference as cr
from tests import cull_cases as cc
from tests import query_cull_cases as qc

SEED = qc.DEFAULT_SEED
TRIANGLE_SCENES = (0, 5)
CPU_QUERIES = ("closest_point", "closest_point_hits", "overlap_boxes", "overlap_triangles", "sweep_spheres", "closest_segment")
# worst |t32 - t64| over closest_reference.t_tolerance, by the family of the nearest instance, where the restatement does not meet the
# tolerance (measured at the default seed; the test asserts twice these and the tolerance itself for every other family)
MEASURED_WORST = {"anisotropic": 80.4, "cancelling": 125.5}
MIN_HIT_SHARE = 0.3           # the threshold of the queries' own test files
# record families whose share of hits is not a property of the family
MAY_MISS = {
    ("overlap_boxes", "box_corner"): "boxes in a corner of an instance's world box and outside its mesh: the tree's boxes are entered, the "
                                     "surface is mostly not touched; that is the family",
}


@pytest.fixture(scope="module")
def all_scenes():
    return list(qc.scenes(SEED))


def test_the_generator_is_deterministic(all_scenes):
    again = list(qc.scenes(SEED))
    other = list(qc.scenes(SEED + 1))
    assert len(all_scenes) == qc.N_SCENES == len(again)
    for a, b, c in zip(all_scenes, again, other):
        assert a.verts.tobytes() == b.verts.tobytes() and a.idx.tobytes() == b.idx.tobytes() and a.ranges == b.ranges
        assert a.instances.tobytes() == b.instances.tobytes() and a.families == b.families
        assert a.instances.tobytes() != c.instances.tobytes()
    sc = all_scenes[2]
    for make in (qc.point_records, qc.sweep_records, qc.box_records, qc.segment_records, qc.triangle_records):
        one, two = make(sc, SEED), make(sc, SEED)
        assert list(one) == list(two)
        for k in one:
            assert one[k][0].tobytes() == two[k][0].tobytes() and len(one[k][0]) >= 128 and one[k][0].dtype == np.float32, k
            assert np.array_equal(one[k][1], two[k][1])


def test_scene_sizes_and_family_counts(all_scenes):
    """6 to 10 instances, at most about 2 500 triangles, a BLAS of 640 triangles; every family at least twice in the set and at least
    twice on the large mesh; scenes 5, 6 and 7 translated by 1e3, 1e4 and 1e5 along (1, 1, 1)"""
    total, large = {f: 0 for f in qc.INSTANCE_FAMILIES}, {f: 0 for f in qc.INSTANCE_FAMILIES}
    for sc in all_scenes:
        n_tris = sum(sc.ranges[sc.mesh_of(i)][2] for i in range(len(sc.instances)))
        assert 6 <= len(sc.instances) <= 10 and n_tris <= 2600, (sc.name, len(sc.instances), n_tris)
        assert sc.ranges[qc.LARGE][2] == 640 and 12 <= sc.ranges[qc.SOUP][2] <= 40 and sc.ranges[qc.CUBE][2] == 12 and sc.ranges[qc.OCTA][2] == 8
        assert len(sc.families) == len(sc.instances) == len(sc.meta)
        for f in qc.INSTANCE_FAMILIES:
            total[f] += len(sc.with_family(f)); large[f] += len(sc.with_family(f, large=True))
        pl = qc.Placement(sc)
        assert np.abs(pl.c - sc.shift).max() < 8.0 and 5.0 < pl.diag < 40.0, (sc.name, pl.c, pl.diag)
    assert [sc.shift for sc in all_scenes] == [0, 0, 0, 0, 0, 1e3, 1e4, 1e5]
    print("instances per family: %s\non the large mesh: %s" % (total, large))
    assert min(total.values()) >= 2 and min(large.values()) >= 2, (total, large)


def test_every_instance_is_of_its_family(all_scenes):
    best_large = 0.0
    for sc in all_scenes:
        conds = []
        for i, fam in enumerate(sc.families):
            r, meta, what = sc.instances[i], sc.meta[i], (sc.name, i, fam)
            M = cc.matrix(r)
            if "void" in fam:
                assert np.isnan(M).sum() == 1, what
                continue
            sv = np.linalg.svd(M[:, :3], compute_uv=False)
            T = qc.world_triangles(sc, i)
            if "singular" in fam:
                assert sv[2] < 1e-6 * sv[0], what
                continue
            # the aspect floor: ten times the contract's needle limit, for every world triangle
            assert qc.aspects(T).min() >= qc.ASPECT_FLOOR, (what, qc.aspects(T).min())
            cond = sv[0] / sv[2]
            conds.append(cond)
            if fam[0] in ("anisotropic", "sheared", "cancelling"):
                assert meta["condition"] / 2 <= cond <= meta["condition"] * 2, (what, cond, meta)
                assert meta["condition"] == meta["target"] / 2 ** meta["halved"], what
                if sc.mesh_of(i) in qc.LARGE_MESHES:
                    best_large = max(best_large, cond)
            if fam[0] == "sheared":       # the columns keep ordinary lengths: the anisotropy is in their angles
                cols = np.linalg.norm(M[:, :3], axis=0)
                assert cols.max() / cols.min() < 2.0, (what, cols)
            if fam[0] == "rigid_dyadic" or fam[0] == "nested":
                L = M[:, :3] * (np.array([-1.0, 1.0, 1.0]) if "mirrored" in fam else 1.0)
                assert np.array_equal(L, np.eye(3) * L[0, 0]) and L[0, 0] * 64 == np.round(L[0, 0] * 64), what
                assert np.array_equal((M[:, 3] - sc.shift) * 4, np.round((M[:, 3] - sc.shift) * 4)), what
            if "mirrored" in fam:
                assert np.linalg.det(M[:, :3]) < 0, what
            elif fam[0] != "masked":
                assert np.linalg.det(M[:, :3]) > 0, what
            if fam[0] in ("tiny", "huge"):
                s = 1e-3 if fam[0] == "tiny" else 1e3
                assert np.allclose(sv, s, rtol=1e-5), what
                size = np.linalg.norm(T.reshape(-1, 3).max(0) - T.reshape(-1, 3).min(0))
                assert (0.5 < size < 10.0) == meta["ordinary"], (what, size)
            if fam[0] == "cancelling":
                # the terms of a row of xform_point exceed the world coordinates (relative to the scene's own translation) 100 times
                v = qc.mesh_triangles(sc.verts, sc.idx, sc.ranges, sc.mesh_of(i)).reshape(-1, 3)
                terms = np.abs(M[:, :3][None] * v[:, None, :]).max(axis=(0, 2))
                world = np.abs(T.reshape(-1, 3) - sc.shift).max(axis=0)
                assert (np.maximum(terms, np.abs(M[:, 3] - sc.shift)) >= 100 * world).any() and terms.max() >= 100 * world.max(), (what, terms, world)
            if fam[0] == "coincident":
                assert sc.instances[meta["twin"]].tobytes() == r.tobytes() and abs(meta["twin"] - i) > 1, what
            if fam[0] == "nested":
                lo, hi = T.reshape(-1, 3).min(0), T.reshape(-1, 3).max(0)
                H = qc.world_triangles(sc, meta["host"]).reshape(-1, 3)
                assert (lo > H.min(0)).all() and (hi < H.max(0)).all(), what
            if fam[0] == "masked":
                assert sc.mask_of(i) == 0 and i == len(sc.instances) - 1, what
                P = np.concatenate([qc.world_triangles(sc, j).reshape(-1, 3) for j in qc.Placement(sc).inst])
                assert (T.reshape(-1, 3).min(0) < P.min(0)).all() and (T.reshape(-1, 3).max(0) > P.max(0)).all(), what
            elif "masked" in fam:
                m = sc.mask_of(i)
                assert m and m & (m - 1) == 0, what
        assert max(conds) >= 100, (sc.name, conds)
    assert best_large >= 500, best_large


def hit_mask(query, ref):
    if query in ("overlap_boxes", "overlap_triangles"):
        return ref[0] > 0
    if query == "closest_point_hits":
        return ref[1] > 0
    h = ref[0] if isinstance(ref, tuple) else ref
    return h["inst"] >= 0


@pytest.mark.parametrize("index", range(qc.N_SCENES))
def test_the_references_alone_referee_the_records(index):
    """per (query, record family) at least 30 % of the records hit something; equidistant points have two or more (inst, prim) at the
    minimal binary32 d2 in at least half of the cases; radius_at_answer yields hits and misses; an answer on a coincident pair names
    the smaller instance index; invalid records are answered by the miss form"""
    w = qc.world(index, SEED)
    sc = w.scene
    for query in CPU_QUERIES + (("closest_triangle",) if index in TRIANGLE_SCENES else ()):
        recs, fam, tgt = w.records(query)
        hit = hit_mask(query, w.reference(query, 0xFF))
        for f in np.unique(fam):
            n, share = int((fam == f).sum()), float(hit[fam == f].mean())
            print("%s %s %-20s %4d records, %.2f hit" % (sc.name, query, f, n, share))
            assert f in ("radius_at_answer", "invalid") or n >= 128, (query, f, n)
            if f == "radius_at_answer":
                assert 0 < hit[fam == f].sum() < n, (query, f)
            elif f != "invalid" and (query, f) not in MAY_MISS:
                assert share >= MIN_HIT_SHARE, (sc.name, query, f, share)
            elif f != "invalid":       # (some of them do reach the surface; the GPU file proves from the counters that boxes are entered)
                assert 0 < share < MIN_HIT_SHARE, (sc.name, query, f, share)
        twins = {i: sc.meta[i]["twin"] for i in sc.with_family("coincident")}
        if query not in ("overlap_boxes", "overlap_triangles", "closest_point_hits"):
            h = w.reference(query, 0xFF)
            h = h[0] if isinstance(h, tuple) else h
            named = h["inst"][h["inst"] >= 0]
            assert all(int(i) < twins[int(i)] for i in named if int(i) in twins), query
            assert not twins or np.isin(named, list(twins)).sum() > 0, (sc.name, query)
    recs, fam, _ = w.records("closest_point")
    eq = recs[fam == "equidistant"]
    adm = np.nonzero(w.S.admitted(0xFF))[0]
    d2, _, _ = cr.tri_d2(tuple(eq[:, k][:, None] for k in range(3)), tuple(w.S.a[adm, k][None] for k in range(3)),
                         tuple(w.S.ab[adm, k][None] for k in range(3)), tuple(w.S.ac[adm, k][None] for k in range(3)))
    with np.errstate(invalid="ignore"):
        ties = ((d2 == np.nanmin(d2, axis=1, keepdims=True)).sum(axis=1) > 1)
    print("%s equidistant: %.2f of the points tie" % (sc.name, ties.mean()))
    assert ties.mean() >= 0.5, ties.mean()
    print("%s reference seconds %s" % (sc.name, {k: round(v, 1) for k, v in w.seconds.items()}))


@pytest.mark.parametrize("index", range(qc.N_SCENES))
def test_point_restatement_against_binary64_under_anisotropy(index):
    """closest_reference.brute32 against brute64 on every scene (each holds anisotropic, sheared or cancelling instances of condition
    100 to 1000): t within closest_reference.t_tolerance, the tolerance tests/test_closest_point.py holds it to on its
    well-conditioned scenes, by the family of the nearest instance.  Measured worst error over the tolerance at the default seed: 0.14
    and less for rigid_dyadic, nested, tiny, huge, coincident, singular and sheared instances (sheared: 0.062 at sigma_min / sigma_max
    1e-3); 80.4 for anisotropic ones (scene 3, the octahedron at condition 1000 whose faces have aspect 1.3e-3; 2.3 on the torus at
    condition 500, 0.11 and less at condition 100 and below); 125.5 for cancelling ones (scene 2, the soup 1000 to 10 000 from the
    object-space origin: xform_point rounds terms of that size; 47 and 78 on the torus; 0.35 and less 1000 and more from the world
    origin, where the tolerance's magnitude term covers it).  A finding about the canonical arithmetic (DESIGN.md §5 "Closest
    points"): MEASURED_WORST, asserted at twice the measurement; every other family is held to the tolerance itself."""
    w = qc.world(index, SEED)
    recs, fam, _ = w.records("closest_point")
    keep = np.isin(fam, qc.POINT_FAMILIES)
    h = w.reference("closest_point", 0xFF)[keep]
    r = cr.brute64(w.S, recs[keep], picked=(h["inst"], h["prim"]))
    assert (h["inst"] >= 0).all()
    err, tol = np.abs(h["t"].astype(np.float64) - r["t"]), cr.t_tolerance(r["t"], r["mag"])
    ifam = np.array([w.scene.families[i][0] for i in r["inst"]])
    beyond = []
    for f in np.unique(ifam):
        ratio = (err / tol)[ifam == f]
        print("%s: nearest instance %-12s %4d points, worst t error %.3g of its bound" % (w.scene.name, f, len(ratio), ratio.max()))
        if ratio.max() > 2 * MEASURED_WORST.get(f, 0.5):
            beyond.append((w.scene.name, f, ratio.max()))
    assert not beyond, beyond


# ---- the other queries' restatements against their binary64 siblings, with the criteria of their own test files -------------------------
ACCURACY_STRIDE = 8           # every eighth generated record of a query (80 to 112 per scene), its invalid and radius records left out
# Where a restatement does not meet its file's criterion on these scenes: the measured worst figure by (query, family of the nearest
# instance), at the default seed; asserted at twice the measurement (everything not listed: the criterion itself).
#   closest_segment: 51.3 bounds for cancelling instances (scene 4, the torus 1000 to 10 000 from the object-space origin; 13.2 in
#     scene 0), 25.9 for anisotropic ones (scene 3, the octahedron at condition 1000 with faces of aspect 1.3e-3; 0.41 and less
#     elsewhere); every other family 0.09 and less.
#   closest_triangle (scenes 0 and 5): 4.09 bounds for cancelling instances (scene 0); every other family 0.075 and less.
#   sweep_spheres: the sandwich holds at the file's K = 16 on every scene and family (nothing listed).
#   overlap_triangles: brute32 and brute64 agree on every pair (nothing listed).
#   overlap_boxes: every disagreeing pair has a binary64 separation of 3e-4 REL and less, but they are 9.74 % of the intersecting or
#     near pairs in scene 0 (1.2 to 7.2 % in scenes 1 to 6) where the file's cap is 1 %: the coplanar_face boxes touch the torus's
#     flat ring and the cube's faces exactly, and binary32 forms the box as centre and half extent, which rounds an exact touch
#     away (DESIGN.md §5 "Box overlaps": why that file keeps its own tie sets small).
MEASURED = {("closest_segment", "cancelling"): 51.3, ("closest_segment", "anisotropic"): 25.9, ("closest_triangle", "cancelling"): 4.09,
            ("overlap_boxes", "share"): 0.0974}


def _subset(w, query):
    recs, fam, _ = w.records(query)
    idx = np.nonzero(~np.isin(fam, ("radius_at_answer", "invalid")))[0][::ACCURACY_STRIDE]
    return recs[idx], fam[idx], idx


def _by_family(w, query, inst, ratio, what):
    """prints the worst ratio per family of the nearest instance and asserts it: 1 (the file's own bound), or twice MEASURED"""
    ifam = np.array([w.scene.families[i][0] if i >= 0 else "none" for i in inst])
    beyond = []
    for f in np.unique(ifam):
        worst = float(np.max(ratio[ifam == f], initial=0.0))
        print("%s %s: nearest instance %-12s %4d records, worst %s %.3g of its bound" % (w.scene.name, query, f, (ifam == f).sum(), what, worst))
        if worst > max(1.0, 2 * MEASURED.get((query, f), 0.0)):
            beyond.append((w.scene.name, query, f, worst))
    assert not beyond, beyond


@pytest.mark.parametrize("index", range(qc.N_SCENES))
def test_segment_restatement_against_binary64(index):
    """segment_reference.brute32 against brute64: |t32 - t64| within tests/test_closest_segment.py's t_bound (K (1e-5 t + 1e-6 M),
    shallow crossings K 2^-12 M), by the family of the nearest instance; see MEASURED for the families beyond it"""
    from tests import segment_reference as sgr, test_closest_segment as tcs
    w = qc.world(index, SEED)
    segs, fam, idx = _subset(w, "closest_segment")
    h = w.reference("closest_segment", 0xFF)[0][idx]
    r = sgr.brute64(w.S, segs, picked=(h["inst"], h["prim"]))
    assert (h["inst"] >= 0).all()
    shallow = tcs.shallow_crossings(w.S, segs, r, h)
    ratio = np.abs(h["t"].astype(np.float64) - r["t"]) / tcs.t_bound(r, shallow)
    _by_family(w, "closest_segment", r["inst"], ratio, "t error")


@pytest.mark.parametrize("index", TRIANGLE_SCENES)
def test_triangle_restatement_against_binary64(index):
    """triangle_distance_reference.brute32 against brute64: |t32 - t64| within tests/test_closest_triangle.py's t_bound, by the family
    of the nearest instance; see MEASURED for the families beyond it"""
    from tests import test_closest_triangle as tct, triangle_distance_reference as tdr
    w = qc.world(index, SEED)
    tris, fam, idx = _subset(w, "closest_triangle")
    h = w.reference("closest_triangle", 0xFF)[0][idx]
    r = tdr.brute64(w.S, tris, picked=(h["inst"], h["prim"]))
    assert (h["inst"] >= 0).all()
    shallow = tct.shallow_touches(w.S, tris, r, h)
    ratio = np.abs(h["t"].astype(np.float64) - r["t"]) / tct.t_bound(r, shallow)
    _by_family(w, "closest_triangle", r["inst"], ratio, "t error")


@pytest.mark.parametrize("index", range(qc.N_SCENES))
def test_sweep_restatement_against_binary64(index):
    """sweep_reference.brute32 in tests/test_sphere_sweep.py's sandwich t64(r + delta) - tau <= t32 <= t64(r - delta) + tau: the smallest
    power of two of the sandwich's constant that holds every record, over the file's K = 16, by the family of the reported instance"""
    from tests import sweep_reference as sr, test_sphere_sweep as tss
    w = qc.world(index, SEED)
    s, fam, idx = _subset(w, "sweep_spheres")
    h = w.reference("sweep_spheres", 0xFF)[idx]
    # (the sandwich's magnitudes and binary64 times cannot take a NaN record: the void instance, which no reference ever names, gets
    # instance 0's transform and mask 0 for this comparison)
    inst = w.scene.instances.copy()
    for i in w.scene.with_family("void"):
        inst[i]["transform"] = inst[0]["transform"]
        inst[i]["custom_index_and_mask"] &= 0x00FFFFFF
    S = cr.Scene(w.scene.verts, w.scene.idx, w.scene.ranges, inst)
    pairs = sr.candidate_pairs(S, s)
    need = np.full(len(s), np.inf)
    for e in range(4, 25, 2):         # K = 16, 64, 256, ...
        sw = tss.sandwich(S, s, pairs, h, 2.0 ** e)
        with np.errstate(invalid="ignore"):
            good = ~sw["ok"] | ((sw["lower"] <= sw["t32"]) & (sw["t32"] <= sw["upper"]))
        need = np.where(good & np.isinf(need), 2.0 ** e / tss.K, need)
        if good.all():
            break
    _by_family(w, "sweep_spheres", h["inst"], need, "sandwich constant")


@pytest.mark.parametrize("query", ["overlap_boxes", "overlap_triangles"])
@pytest.mark.parametrize("index", range(qc.N_SCENES))
def test_overlap_restatements_against_binary64(index, query):
    """brute32 against brute64 pair by pair, the criterion of tests/test_overlap_boxes.py and tests/test_triangle_overlaps.py: every pair
    they disagree on has a binary64 separation within REL of zero (printed and asserted as |separation| / REL by the pair's instance
    family), and such pairs are at most 1 % of the intersecting-or-near pairs"""
    from tests import overlap_reference as orf, triangle_overlap_reference as tor
    from tests.query_reference import REL
    w = qc.world(index, SEED)
    q, fam, idx = _subset(w, query)
    mod = orf if query == "overlap_boxes" else tor
    keep = fam != "degenerate"        # (zero-area queries against the flat instance are left open by the contract)
    q = q[keep]
    bi, ti = mod.surviving_pairs(w.tris, q)
    c32 = mod.candidates32(w.tris, q, bi, ti)
    s64 = mod.separation64(w.tris, q, bi, ti)
    differ = c32 != (s64 <= 0)
    pool = (s64 <= 0) | (np.abs(s64) <= REL)
    print("%s %s: %d pairs, %d intersecting or near, %d differ" % (w.scene.name, query, len(bi), pool.sum(), differ.sum()))
    share = differ.sum() / max(pool.sum(), 1)
    print("%s %s: the disagreeing pairs are %.4f of the intersecting or near ones" % (w.scene.name, query, share))
    _by_family(w, query, w.S.inst[ti[differ]], np.abs(s64[differ]) / REL, "|separation| of a disagreeing pair")
    assert share <= max(0.01, 2 * MEASURED.get((query, "share"), 0.0)), (differ.sum(), pool.sum())
