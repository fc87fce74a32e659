"""The frame path's conservative culls against the plain walk and the oracle, on the seeded adversarial cases of tests/cull_cases.py
(run with `-m gpu` on a real MI355X).  rt_api.h says of the switches "Results do not depend on any of them": for every case the frame
with every cull off (PLAIN) equals the oracle's bit for bit, ray counts per class included, and every other configuration — all
defaults over three consecutive frames (the kept light records are built, then used), each cull alone over PLAIN, device instance
records, the host's tree builder, band shards, a frame batch — equals PLAIN bit for bit.  The last test proves from the counters
that the culls were engaged, family by family.  One test is one scene with its ~16 poses."""
import numpy as np
import pytest

from tests import cull_cases as cc, scenes
from tests.exact import assert_frame_equals_oracle, frame_mismatch
from vulkan_raytracing_amd import RtContext, tiling

pytestmark = pytest.mark.gpu
SEED = cc.DEFAULT_SEED

PLAIN = dict(primary_cover=0, entry_points=0, shadow_entry=0, pixel_beams=0, dead_shadow_rays=0, fused_shade=0, jitter_table=0, tail_kernel=0)
DEFAULT = dict(primary_cover=1, entry_points=1, shadow_entry=2, pixel_beams=1, dead_shadow_rays=1, fused_shade=1, jitter_table=1, tail_kernel=1)
# one cull at a time over PLAIN, so that a failure names its cull (counting frames where the engagement proof reads node visits)
SINGLE = (("primary_cover", dict(primary_cover=1), True),
          ("primary_cover + entry_points, shadow_entry 0", dict(primary_cover=1, entry_points=1, shadow_entry=0), True),
          ("primary_cover + entry_points, shadow_entry 1", dict(primary_cover=1, entry_points=1, shadow_entry=1), False),
          ("pixel_beams", dict(pixel_beams=1), False),
          ("pixel_beams + fused_shade", dict(pixel_beams=1, fused_shade=1), False),
          ("dead_shadow_rays", dict(dead_shadow_rays=1), False))
BATCH_SIZE = (64, 40)

# Engagement conditions a family does not have to meet, with the reason (test_the_culls_were_engaged lists what it skips; everything
# else is asserted for every family).
NOT_ENGAGED = {
    ("near_singular", "mask"): "rt_api.cpp refuses the basis of every second case (|det| half the threshold: no mask at all), and the rays of the "
                               "others fan out in one plane through the anchor, where every tile the root boxes cover has a frontier box too",
    ("far_origin_closeup", "mask"): "by design since k_cover carries the rounding of world coordinates (DESIGN.md §5): 300 and more from the origin, a box "
                                    "0.003 .. 0.02 in front of the camera is not safely in front of the camera plane (az <= 2 ec): whole-frame flag",
    ("far_origin", "mask"): "the light family of the far_origin_closeup cameras: see there",
    ("long_lens", "mask"): "the lens frames one object: behind it the floor fills every tile, and without the floor the boxes of the TLAS root are "
                           "that object's own box",
    ("long_lens", "settled"): "the lens frames the anchor or the tilted instance, the scene's mirror and glass: the diffuse surface in view is the "
                              "floor, which these lights see from its front",
    ("off_screen_edge", "mask"): "the camera stands two to four box sizes from the anchor it straddles: the anchor's and the floor's frontier "
                                 "boxes cover every tile that the TLAS root's boxes cover",
    ("wide", "settled"): "settling is decided by the light's side of a diffuse surface; in these views the objects are a few pixels each and "
                         "none of the family's lights stood behind a diffuse surface the camera saw",
    ("at_camera", "settled"): "a light at the camera is on the visible side of everything the camera sees: diffuse is never exactly 0",
    ("far", "kept_light_records"): "from 1e4 away the whole scene falls into one or two tiles of the light's cube: a record cannot start "
                                   "deeper than the TLAS root there, and reading it costs visits",
}


def _configure(c, params):
    for k, v in params.items():
        c.set_param(k, v)


@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_host_trees():
    """a second context whose trees the host's binned-SAH builder makes ("blas_builder" 0): other tree shapes under k_entry"""
    c = RtContext(0)
    c.set_param("blas_builder", 0)
    yield c
    c.close()


def _counts(st):
    return (int(st.rays_primary), int(st.rays_secondary), int(st.rays_shadow))


class _Report:
    """differences of one scene, each with everything needed to reproduce it"""

    def __init__(self, scene):
        self.scene, self.lines = scene, []

    def compare(self, pose, config, img, counts, want_img, want_counts):
        bad = frame_mismatch(img, want_img)
        if len(bad) == 0 and counts == want_counts:
            return
        self.lines.append("seed %d, %r, configuration [%s]: %d pixels differ from the reference frame (PLAIN unless named), first (x, y) %s; rays %s against %s"
                          % (SEED, pose, config, len(bad), bad[:6].tolist(), counts, want_counts))

    def add(self, pose, config, text):
        self.lines.append("seed %d, %r, configuration [%s]: %s" % (SEED, pose, config, text))


def _shards(c, W, H, band, n):
    import torch
    rows_max = tiling.max_shard_rows(H, band, n)
    parts = []
    for s in range(n):
        buf = torch.zeros((rows_max, W, 4), dtype=torch.float32, device="cuda:0")
        c.trace_shard(W, H, band, s, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
        c.synchronize()
        parts.append(buf.cpu().numpy())
    return tiling.assemble(parts, H, W, band)


def _batch(c, sc, three, report):
    """three cameras (and lights) of three families as ONE rt_set_batch against their single frames"""
    import torch
    W, H = BATCH_SIZE
    us = []
    for p in three:
        u = sc.uniforms.copy()
        for f in ("position", "right", "up", "forward", "light_position"):
            u[0][f] = p.uniforms[0][f]
        us.append(u)
    singles = []
    c.set_instances(sc.instances)
    for u in us:
        c.set_uniforms(u)
        img, st = c.trace(W, H)
        singles.append((img, _counts(st)))
    K = len(us)
    c.set_batch(np.stack([sc.instances] * K), np.concatenate(us))
    try:
        buf = torch.zeros((K, H, W, 4), dtype=torch.float32, device="cuda:0")
        c.trace_shard_batch(W, H, 8, 0, 1, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
        c.synchronize()
        st = c.stats()
        out = buf.cpu().numpy()
    finally:
        c.set_instances(sc.instances)     # (a single frame's records again: the batch is dropped)
        c.set_uniforms(us[0])
    for k, p in enumerate(three):
        report.compare(p, "frame %d of a batch of %d at %dx%d against its single frame, defaults" % (k, K, W, H), out[k], singles[k][1], singles[k][0], singles[k][1])
    total = tuple(sum(s[1][k] for s in singles) for k in range(3))
    if _counts(st) != total:
        report.add(three[0], "a batch of %d at %dx%d, defaults" % (K, W, H), "rays %s, the single frames' sum %s" % (_counts(st), total))


def _run_scene(c, c_host, sc):
    """renders every case of the scene in every configuration; returns (report, per-case counters)"""
    import torch
    report, rows = _Report(sc), []
    sp = scenes.ScenePair(sc.paths, sc.instances, sc.uniforms, sky=sc.sky, ctx=c)
    sp.set_instance_types(sc.types)
    c_host.upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
    c_host.set_instance_types(sc.types)
    c_host.set_skybox(sc.sky)
    oracle_frames = {}

    def accept(p):
        sp.orc.set_instances([p.instances[i].tobytes() for i in range(len(p.instances))])
        sp.orc.set_uniforms(p.uniforms.tobytes())
        oracle_frames[p.name] = sp.orc.render(p.W, p.H)
        return bool(np.isfinite(oracle_frames[p.name][0]).all())

    poses = list(cc.poses(sc, SEED, accept=accept))
    try:
        for i, p in enumerate(poses):
            W, H = p.W, p.H
            if p.name not in oracle_frames:
                accept(p)
            sp.set_instances(p.instances); sp.set_uniforms(p.uniforms)        # (the oracle stays in this state for exact.py's arbitration)
            ref, rc = oracle_frames[p.name]
            # ---- PLAIN == the oracle
            _configure(c, PLAIN)
            plain, st = c.trace(W, H)
            plain_counts, row = _counts(st), dict(pose=p, closest_plain=int(st.closest_rays))
            try:
                assert_frame_equals_oracle(plain, sp.orc, W, H, ref=ref)
            except AssertionError as e:
                report.add(p, "PLAIN against the oracle", str(e))
            if plain_counts != tuple(int(x) for x in rc):
                report.add(p, "PLAIN against the oracle", "rays %s, the oracle's %s" % (plain_counts, rc.tolist()))
            # ---- one cull at a time over PLAIN
            for name, params, counting in SINGLE:
                _configure(c, PLAIN); _configure(c, params)
                img, st = c.trace(W, H, counting=counting)
                report.compare(p, name, img, _counts(st), plain, plain_counts)
                if name == "primary_cover":
                    row["visits_cover"] = int(st.node_visits)
                elif counting:
                    row["visits_entry"] = int(st.node_visits)
            # ---- every default, three consecutive frames: the kept light records are built, then used
            _configure(c, DEFAULT)
            for frame in range(3):
                img, st = c.trace(W, H)
                report.compare(p, "defaults, frame %d of 3" % (frame + 1), img, _counts(st), plain, plain_counts)
            row["closest_default"] = int(st.closest_rays); row["untraced"] = int(st.rays_shadow_untraced); row["shadow"] = plain_counts[2]
            img, st = c.trace(W, H, counting=True)
            report.compare(p, "defaults, a fourth (counting) frame", img, _counts(st), plain, plain_counts)
            row["shadow_visits_kept"] = int(st.node_visits_shadow)
            if i % 3 == 0:
                report.compare(p, "defaults, band shards (8, 3)", _shards(c, W, H, 8, 3), plain_counts, plain, plain_counts)
                t = torch.from_numpy(np.ascontiguousarray(p.instances).view(np.uint8).reshape(-1, 64).copy()).to("cuda:0")
                torch.cuda.current_stream().synchronize()
                c.set_instances_device(t)
                for frame in range(2):
                    img, st = c.trace(W, H)
                    report.compare(p, "defaults, rt_set_instances_device, frame %d" % (frame + 1), img, _counts(st), plain, plain_counts)
                c.set_instances(p.instances)
                _configure(c_host, DEFAULT)
                c_host.set_instances(p.instances); c_host.set_uniforms(p.uniforms)
                for frame in range(2):
                    img, st = c_host.trace(W, H)
                    report.compare(p, "defaults, blas_builder 0, frame %d" % (frame + 1), img, _counts(st), plain, plain_counts)
            c.set_param("shadow_entry", 0)           # (drops the kept records)
            img, st = c.trace(W, H, counting=True)
            report.compare(p, "defaults but shadow_entry 0 (counting)", img, _counts(st), plain, plain_counts)
            row["shadow_visits_off"] = int(st.node_visits_shadow)
            rows.append(row)
        # ---- one frame batch of three cameras from three different families
        _configure(c, DEFAULT)
        three, seen = [], set()
        for p in poses:
            if p.families[0] not in seen and len(p.instances) == len(sc.instances) and np.array_equal(p.instances, sc.instances):
                three.append(p); seen.add(p.families[0])
            if len(three) == 3:
                break
        assert len(three) == 3
        _batch(c, sc, three, report)
    finally:
        _configure(c, DEFAULT)
    return report, rows


@pytest.fixture(scope="module")
def results(ctx, ctx_host_trees):
    """scene index -> (report, counters), rendered once"""
    done = {}
    by_index = {sc.index: sc for sc in cc.scenes(SEED)}

    def get(index):
        if index not in done:
            try:
                done[index] = _run_scene(ctx, ctx_host_trees, by_index[index])
            except AssertionError:
                raise
            except Exception as e:       # an error of the library (a GPU fault among them): nothing more is started on the GPU
                pytest.exit("scene %d (seed %d): %s: %s" % (index, SEED, type(e).__name__, e), returncode=3)
        return done[index]

    return get


@pytest.mark.parametrize("index", range(cc.N_SCENES))
def test_no_cull_changes_a_frame(results, index):
    """every case of the scene: PLAIN == the oracle; defaults x 3 frames, each cull alone, device records, host-built trees, band
    shards and a frame batch == PLAIN, bit for bit with equal ray counts per class"""
    report, rows = results(index)
    assert len(rows) >= cc.N_POSES
    assert not report.lines, "%d differences\n%s" % (len(report.lines), "\n".join(report.lines[:12]))


ENGAGEMENT = (("mask", "the coverage mask removed rays somewhere: closest_rays(defaults) < closest_rays(PLAIN)"),
              ("records", "entry records save node visits: counting frames with primary_cover + entry_points against primary_cover alone"),
              ("kept_light_records", "the kept light records save shadow node visits: defaults' fourth frame against shadow_entry 0"),
              ("settled", "some shadow rays were settled and not walked: rays_shadow_untraced > 0"))


def test_the_culls_were_engaged(results):
    """Without this the module could pass with every cull switched off.  Per family, summed over its cases (see ENGAGEMENT); and among
    the in_box / on_box_plane cameras somewhere closest_rays(defaults) == closest_rays(PLAIN) > 0: the whole-frame flag.  An entry of
    NOT_ENGAGED whose condition is met after all is an error too.  Measured on an MI355X at the default seed (ratios of the sums):

    family                   cases  mask removed rays in  closest_rays defaults/PLAIN  node_visits records/none  shadow visits kept/off  settled
    at_camera                   21                     4                       0.946                     0.617                   0.095        0
    axis_view                   15                    10                       0.852                     0.485                   0.230     6156
    cube_diagonal               22                     4                       0.987                     0.540                   0.197       83
    far                         23                     6                       0.951                     0.384                   1.578       26
    far_origin                  15                     0                       1.000                     0.684                   0.506   148667
    far_origin_closeup          15                     0                       1.000                     0.684                   0.506   148667
    grazing                     15                     4                       0.989                     0.609                   0.353     4473
    in_box                      37                     6                       0.940                     0.684                   0.338      154
    in_mesh                     37                     9                       0.957                     0.631                   0.071     6159
    left_handed                 15                     3                       0.982                     0.460                   0.191       13
    long_lens                   15                     0                       1.000                     0.688                   0.273        0
    near_singular               15                     0                       1.000                     0.841                   0.680      108
    near_surface                23                     2                       0.995                     0.670                   0.038   110803
    off_screen_edge             15                     0                       1.000                     0.294                   0.258   106430
    on_box_plane                38                    15                       0.868                     0.521                   0.186      562
    outside                     21                     5                       0.919                     0.538                   0.390        2
    shell                       14                     8                       0.598                     0.446                   0.155       47
    subpixel_on_tile_corner     15                     5                       0.952                     0.523                   0.104      554
    wide                        15                     5                       0.875                     0.146                   0.056        0
    whole-frame flag cases among in_box / on_box_plane: 21
    """
    fam = {}
    whole_frame = 0
    for index in range(cc.N_SCENES):
        for row in results(index)[1]:
            p = row["pose"]
            if p.families[0] in ("in_box", "on_box_plane") and row["closest_default"] == row["closest_plain"] > 0:
                whole_frame += 1
            for f in p.families:
                t = fam.setdefault(f, dict(cases=0, mask=0, closest_plain=0, closest_default=0, visits_cover=0, visits_entry=0,
                                           shadow_visits_off=0, shadow_visits_kept=0, untraced=0, shadow=0))
                t["cases"] += 1; t["mask"] += int(row["closest_default"] < row["closest_plain"])
                for k in ("closest_plain", "closest_default", "visits_cover", "visits_entry", "shadow_visits_off", "shadow_visits_kept", "untraced", "shadow"):
                    t[k] += row[k]
    lines = ["%-24s %s" % (f, " ".join("%s %d" % kv for kv in t.items())) for f, t in sorted(fam.items())]
    print("\n".join(["engagement per family (seed %d)" % SEED] + lines + ["whole-frame flag cases among in_box / on_box_plane: %d" % whole_frame]))
    assert set(fam) == set(cc.CAMERA_FAMILIES) | set(cc.LIGHT_FAMILIES)
    missed = []
    for f, t in sorted(fam.items()):
        met = dict(mask=t["mask"] > 0 and t["closest_default"] < t["closest_plain"], records=t["visits_entry"] < t["visits_cover"],
                   kept_light_records=t["shadow_visits_kept"] < t["shadow_visits_off"], settled=t["untraced"] > 0)
        for key, what in ENGAGEMENT:
            if (f, key) in NOT_ENGAGED:
                print("not required of %s: %s (%s)" % (f, key, NOT_ENGAGED[(f, key)]))
                if met[key]:
                    missed.append("%s: listed in NOT_ENGAGED for [%s], which it meets: take it off the list\n    %s" % (f, key, t))
            elif not met[key]:
                missed.append("%s: %s\n    %s" % (f, what, t))
    assert whole_frame > 0, "no in_box / on_box_plane camera took the whole-frame flag"
    assert not missed, "\n".join(missed)
