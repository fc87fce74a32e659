"""GPU parity tests (run with `-m gpu` on a real MI355X).  Every call goes through the C ABI of
librt_mi355x.so; the oracle is only the checker.

Bars: hit records equal the oracle's in every field (t, u, v, prim, inst) bit for bit, on every ray (integer/index work and
the canonical arithmetic of DESIGN.md); images equal the oracle's frame bit for bit, every pixel and every channel
(tests/exact.py: no tolerance; a failure names the pixels and says whether the GPU or the oracle's BVH mode agrees with
the oracle's brute-force re-render).  The one exception is the SPIR-V fixture comparison, whose recorded rays differ
from the kernels' by an ulp."""
import os

import numpy as np
import pytest

from tests import scenes
from tests.exact import assert_frame_equals_oracle, assert_hits_equal_oracle
from vulkan_raytracing_amd import RtContext, host, tiling, workloads
from vulkan_raytracing_amd.api import RtError

pytestmark = pytest.mark.gpu
RES = scenes.RES


@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_alt():
    """A context of librt_mi355x_alt.so: the product sources compiled with -DRT_ALT_KERNELS, i.e. WITH the traversal kernels that
    measured slower and are not shipped (k_packet, the quad/BVH4 kernel, 4-ary records, tile blobs, shadow beams).  Loaded next to the
    product library."""
    c = RtContext(0, variant="alt")
    yield c
    c.close()


def test_device_is_gfx950(ctx):
    assert "gfx950" in ctx.device_info


def test_intersect_closest_and_any_teapot_cube(ctx):
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 1, 0, 1, 1, ctx=ctx)
    rays = scenes.random_rays(20000, seed=11)
    g, _ = ctx.intersect(rays)
    o = sp.orc.intersect(rays, use_bvh=False)  # brute force: independent of any BVH
    assert (o["inst"] >= 0).mean() > 0.3
    assert np.array_equal(g["inst"], o["inst"]) and np.array_equal(g["prim"], o["prim"])
    assert np.array_equal(g["t"].view(np.uint32), o["t"].view(np.uint32))
    assert np.array_equal(g["u"].view(np.uint32), o["u"].view(np.uint32)) and np.array_equal(g["v"].view(np.uint32), o["v"].view(np.uint32))
    sh = rays.copy(); sh[:, 7] = 18.0
    ga, _ = ctx.intersect(sh, any_hit=True)
    oa = sp.orc.intersect(sh, use_bvh=False)
    assert np.array_equal(ga["inst"] >= 0, oa["inst"] >= 0)


def test_intersect_edge_cases(ctx):
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 1, 0, 1, 1, ctx=ctx)
    # empty batch, single ray, a batch that is not a multiple of 64, axis-parallel rays, tmin/tmax windows
    g, _ = ctx.intersect(np.zeros((0, 8), np.float32))
    assert len(g) == 0
    rays = np.array([[0, 0, 20, 0.001, 0, 0, -1, 10000.0],      # shared edge of two cube triangles (tie rule)
                     [0, 0, 20, 0.001, 0, 0, 1, 10000.0],       # pointing away
                     [0, 0, 20, 14.5, 0, 0, -1, 10000.0],       # tmin past the first surface: back face of the cube (no culling)
                     [0, 0, 20, 0.001, 0, 0, -1, 13.9],         # tmax before the first surface
                     [0.3, 20, 5.2, 0.001, 0, -1, 0, 10000.0],  # straight down on the cube top
                     [50, 50, 50, 0.001, 1, 0, 0, 10000.0]], np.float32)
    g, _ = ctx.intersect(rays)
    o = sp.orc.intersect(rays, use_bvh=False)
    assert np.array_equal(g, o)
    assert g["t"][0] == 14.0 and g["prim"][0] == 0 and g["inst"][1] == -1 and g["inst"][3] == -1 and g["t"][2] == 16.0
    odd = scenes.random_rays(64 * 3 + 17, seed=5)
    g, _ = ctx.intersect(odd)
    assert np.array_equal(g, sp.orc.intersect(odd, use_bvh=False))


MESHES = ("standin", "limbs")   # the star-shaped geodesic blob of round 1 and the non-star-shaped figure with limbs


@pytest.mark.parametrize("mesh", MESHES)
def test_intersect_armadillo_standin_vs_oracle_bvh(ctx, mesh):
    """346 k-triangle class mesh: GPU BVH traversal vs the oracle's own (independent) BVH."""
    arm, label = host.armadillo_path(RES, kind=mesh)
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 1, 0, 3, 1, ctx=ctx)
    rays = scenes.random_rays(30000, seed=21, target_radius=5.0)
    g, st = ctx.intersect(rays, counting=True)
    o = assert_hits_equal_oracle(g, sp.orc, rays)     # every field of every record, bit for bit (differences re-resolved by brute force)
    assert (o["inst"] >= 0).mean() > 0.3
    assert st.node_visits > 0 and st.tri_tests > 0
    # a brute-force spot check on a few hundred rays (O(N) each)
    sub = rays[:300]
    ob = sp.orc.intersect(sub, use_bvh=False)
    assert np.array_equal(g[:300]["prim"], ob["prim"]) and np.array_equal(g[:300]["t"].view(np.uint32), ob["t"].view(np.uint32))
    assert np.array_equal(g[:300].view(np.uint8), ob.view(np.uint8))


def test_cfg1_cube_scene_image(ctx):
    """BASELINE config 1 shape (cube_scene, 256x256, depth 1, spp 1) on the HIP path."""
    inst = [host.make_instance(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), 0, 0)]
    u = host.default_uniforms(max_bounce_count=0, samples_per_pixel=1, center_object_type=0, orbiting_object_type=0)
    sp = scenes.ScenePair([os.path.join(RES, "cube_scene.obj")], inst, u, sky=scenes.synthetic_skybox(64), ctx=ctx)
    gpu, st = ctx.trace(256, 256)
    ref, rc = sp.orc.render(256, 256)
    assert_frame_equals_oracle(gpu, sp.orc, 256, 256, ref=ref)
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))


def test_frames_match_committed_golden_hashes(ctx):
    """The HIP path against the committed fixtures (tests/golden/oracle_images.json: SHA-256 of frames the oracle
    rendered, made by tests/golden/make_oracle_images.py): identical bytes, identical ray counts — no oracle run here."""
    import hashlib
    import importlib.util
    import json
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_oracle_images", os.path.join(here, "make_oracle_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = json.load(open(os.path.join(here, "oracle_images.json")))
    for name, (sp, W, H) in mod.cases().items():
        scenes.ScenePair(sp.geom_paths, sp.instances, sp.uniforms, sky=sp.sky, ctx=ctx)   # same inputs, uploaded to the GPU context
        img, st = ctx.trace(W, H)
        assert hashlib.sha256(np.ascontiguousarray(img, np.float32).tobytes()).hexdigest() == want[name]["sha256"], name
        assert [st.rays_primary, st.rays_secondary, st.rays_shadow] == want[name]["rays"], name


@pytest.mark.parametrize("center_type,orbit_type,max_bounce", [(1, 0, 1), (2, 0, 3), (1, 1, 5), (0, 2, 2)])
def test_cfg2_teapot_cube_image(ctx, center_type, orbit_type, max_bounce):
    """BASELINE config 2 scene (teapot + orbiting cube) at reduced size; mirror, refractive, diffuse mixes."""
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), center_type, orbit_type, max_bounce, 4,
                                 sky=scenes.synthetic_skybox(128), ctx=ctx, time_param=0.35)
    W, H = 320, 180
    gpu, st = ctx.trace(W, H)
    ref, rc = sp.orc.render(W, H)
    assert_frame_equals_oracle(gpu, sp.orc, W, H, ref=ref)
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))
    assert st.rays_secondary > 0


@pytest.mark.parametrize("mesh", MESHES)
def test_cfg3_armadillo_image_small(ctx, mesh):
    """BASELINE config 3 scene (teapot mirror + armadillo stand-in diffuse, depth 4 + shadow rays), 240x136."""
    arm, _ = host.armadillo_path(RES, kind=mesh)
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 1, 0, 3, 4, sky=scenes.synthetic_skybox(128), ctx=ctx)
    W, H = 240, 136
    gpu, st = ctx.trace(W, H)
    ref, rc = sp.orc.render(W, H)
    assert_frame_equals_oracle(gpu, sp.orc, W, H, ref=ref)
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))
    assert st.rays_shadow > 0


def test_cfg5_instanced_ring_image(ctx):
    """BASELINE config 5 shape: 16 instances of one BLAS under one TLAS (two-level BVH)."""
    sp = scenes.ring_scene(os.path.join(RES, "teapot.obj"), 16, 10.0, 3, 2, sky=scenes.synthetic_skybox(64), ctx=ctx,
                           center_path=os.path.join(RES, "cube.obj"))
    W, H = 256, 144
    gpu, st = ctx.trace(W, H)
    ref, rc = sp.orc.render(W, H)
    assert_frame_equals_oracle(gpu, sp.orc, W, H, ref=ref)
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))


def test_tlas_refit_equals_rebuild(ctx):
    """rt_set_instances(update=1) (Vulkan UPDATE mode, src/main.cpp:2853-2861) == fresh build."""
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 1, 0, 2, 2, sky=scenes.synthetic_skybox(64), ctx=ctx)
    anim = host.SceneAnimation()
    W, H = 200, 120
    for k in range(3):
        anim.animate(0.2 * (k + 1))
        inst = anim.instances((0, 1))
        sp.set_instances(inst, update=True)
        refit, _ = ctx.trace(W, H)
        ctx.set_instances(inst, update=False)
        rebuilt, _ = ctx.trace(W, H)
        assert np.array_equal(refit, rebuilt)
        ref, _ = sp.orc.render(W, H)
        assert_frame_equals_oracle(refit, sp.orc, W, H, ref=ref)


def test_sharded_equals_full_frame_bit_exact(ctx):
    """N logical shards on one device == the 1-GPU frame, bit for bit (SURVEY.md §4 multi-GPU row)."""
    import torch
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 1, 0, 2, 2, sky=scenes.synthetic_skybox(64), ctx=ctx)
    W, H = 328, 203  # ragged: not multiples of 8
    full, _ = ctx.trace(W, H)
    for n in (2, 3, 8):
        rows_max = tiling.max_shard_rows(H, tiling.BAND_ROWS, n)
        shards = []
        for s in range(n):
            buf = torch.zeros((rows_max, W, 4), dtype=torch.float32, device="cuda:0")
            ctx.trace_shard(W, H, tiling.BAND_ROWS, s, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
            ctx.synchronize()
            torch.cuda.synchronize()
            assert ctx.shard_rows(H, tiling.BAND_ROWS, s, n) == tiling.shard_rows(H, tiling.BAND_ROWS, s, n)
            shards.append(buf.cpu().numpy())
        out = tiling.assemble(shards, H, W, tiling.BAND_ROWS)
        assert np.array_equal(out, full)
    # band heights other than the tile height (general row mapping of k_raygen) and an odd shard count
    for band, n in ((5, 3), (16, 2), (3, 5)):
        rows_max = tiling.max_shard_rows(H, band, n)
        shards = []
        for s in range(n):
            buf = torch.zeros((rows_max, W, 4), dtype=torch.float32, device="cuda:0")
            ctx.trace_shard(W, H, band, s, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
            ctx.synchronize()
            shards.append(buf.cpu().numpy())
        assert np.array_equal(tiling.assemble(shards, H, W, band), full)


@pytest.mark.parametrize("spp", [3, 5, 7])
def test_sample_counts_that_do_not_fill_a_workgroup(ctx, spp):
    """k_raygen packs up to 4 samples of a tile into one workgroup: sample counts that are not multiples of 4, at a
    frame size that is not a multiple of the 8x8 tile, against the oracle."""
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 1, 0, 2, spp, sky=scenes.synthetic_skybox(64), ctx=ctx)
    W, H = 75, 37
    gpu, st = ctx.trace(W, H)
    ref, rc = sp.orc.render(W, H)
    assert_frame_equals_oracle(gpu, sp.orc, W, H, ref=ref)
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))


@pytest.mark.parametrize("mesh", MESHES)
def test_full_size_properties_cfg3(ctx, mesh):
    """At BASELINE config 3 size (1920x1080, depth 4, spp 4) the oracle is too slow for a full
    frame, so check size-independent properties: determinism across runs, alpha == 1, ray
    bookkeeping, an oracle-rendered band of rows, and sharded == unsharded on a band subset."""
    arm, _ = host.armadillo_path(RES, kind=mesh)
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 1, 0, 3, 4, sky=scenes.synthetic_skybox(256), ctx=ctx)
    W, H = 1920, 1080
    a, st = ctx.trace(W, H)
    b, st2 = ctx.trace(W, H)
    assert np.array_equal(a, b)
    assert np.all(a[..., 3] == 1.0) and np.isfinite(a).all()
    assert st.rays_primary == W * H * 4 and st.rays_total == st2.rays_total
    assert st.rays_secondary > 0 and st.rays_shadow > 0
    y0, y1 = 536, 544
    assert_frame_equals_oracle(a, sp.orc, W, H, y0=y0, y1=y1)


def test_error_behaviour(ctx):
    """Status codes instead of the reference's exceptions (src/main.cpp:138-147)."""
    from vulkan_raytracing_amd.api import RtError
    c = RtContext(0)
    with pytest.raises(RtError) as e:
        c.trace(16, 16)
    assert e.value.code == 2  # RT_ERR_NOT_READY: uniforms/geometry missing
    with pytest.raises(RtError):
        c.upload_geometry(np.zeros(6, np.float32), np.array([0, 1, 2], np.uint32), [(0, 0, 1)])  # index out of range
    with pytest.raises(RtError):
        RtContext(99)
    c.close()


def test_frames_in_flight_async_entry_points(ctx):
    """rt_trace_async / rt_trace_wait (submit + fence of src/main.cpp:2905-2967): same pixels and counters as the
    blocking rt_trace, several contexts pending at once, and the call-order errors."""
    paths = (os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"))
    W, H = 200, 120
    sp = scenes.two_object_scene(paths[0], paths[1], 2, 1, 4, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.3)
    ref, st_ref = ctx.trace(W, H)
    with pytest.raises(RtError):
        ctx.trace_wait()                      # nothing submitted
    others = [RtContext(0) for _ in range(2)]
    try:
        for c in others:
            scenes.two_object_scene(paths[0], paths[1], 2, 1, 4, 2, sky=scenes.synthetic_skybox(64), ctx=c, time_param=0.3)
        ring = [ctx] + others
        for _ in range(3):                    # three rounds, three frames pending each time
            for c in ring:
                c.trace_async(W, H)
            with pytest.raises(RtError):
                ring[0].trace_async(W, H)     # one pending frame per context
            # rt_set_instances never disturbs the frame in flight: the records are double-buffered, the pending frame keeps
            # the transforms it was submitted with (the reference would block on the frame's fence here, src/main.cpp:772-778)
            moved_anim = host.SceneAnimation(); moved_anim.animate(1.1)
            ring[0].set_instances(moved_anim.instances((0, 1)), update=True)
            for c in ring:
                img, st = c.trace_wait()
                assert np.array_equal(img, ref)
                assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (st_ref.rays_primary, st_ref.rays_secondary, st_ref.rays_shadow)
            ring[0].set_instances(sp.instances, update=True)       # back for the next round
        # 8-bit surface-format output (src/main.cpp:1899): clamp, x255, round — through both the blocking and the async entry
        try:
            ctx.set_param("output_rgba8", 1)
            want = (np.clip(ref, 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
            img8, _ = ctx.trace(W, H)
            assert img8.dtype == np.uint8 and np.array_equal(img8, want)
            ctx.trace_async(W, H)
            img8b, _ = ctx.trace_wait()
            assert np.array_equal(img8b, want)
        finally:
            ctx.set_param("output_rgba8", 0)
    finally:
        for c in others:
            c.close()


def test_trace_variants_are_result_identical(ctx, ctx_alt):
    """BVH2/one-lane-per-ray, BVH4/four-lanes-per-ray and 4-ary-record/one-lane kernels: identical hit records and images.  The
    alternatives live in librt_mi355x_alt.so only; the product library refuses them, and its frames equal the alt build's."""
    with pytest.raises(RtError):
        ctx.set_param("trace_variant", 2)
    with pytest.raises(RtError):
        ctx.set_param("packet_trace", 1)
    for name in ("tile_blobs", "shadow_beams"):
        with pytest.raises(RtError):
            ctx.set_param(name, 1)
        ctx.set_param(name, 0)
    arm, _ = host.armadillo_path(RES)
    scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 2, 1, 4, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.6)
    product_img, product_st = ctx.trace(256, 144)
    product_rays = (product_st.rays_primary, product_st.rays_secondary, product_st.rays_shadow)
    ctx = ctx_alt
    arm, _ = host.armadillo_path(RES)
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 2, 1, 4, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.6)
    rays = scenes.random_rays(40000, seed=33, target_radius=6.0)
    out = {}
    try:
        for v in (0, 1, 2):
            ctx.set_param("trace_variant", v)
            g, _ = ctx.intersect(rays)
            sh = rays.copy(); sh[:, 7] = 17.0
            ga, _ = ctx.intersect(sh, any_hit=True)
            img, st = ctx.trace(256, 144)
            out[v] = (g, ga["inst"] >= 0, img, (st.rays_primary, st.rays_secondary, st.rays_shadow))
    finally:
        ctx.set_param("trace_variant", 0)
    assert np.array_equal(out[0][2], product_img) and out[0][3] == product_rays
    for v in (1, 2):
        assert np.array_equal(out[0][0], out[v][0])
        assert np.array_equal(out[0][1], out[v][1])
        assert np.array_equal(out[0][2], out[v][2]) and out[0][3] == out[v][3]
    o = assert_hits_equal_oracle(out[0][0], sp.orc, rays)
    for v in (1, 2):
        assert_hits_equal_oracle(out[v][0], sp.orc, rays, ref=o)
    ob = sp.orc.intersect(rays[:300], use_bvh=False)     # and a brute-force spot check
    assert np.array_equal(out[0][0][:300].view(np.uint8), ob.view(np.uint8))


def test_bench_two_ranks_on_one_gpu_reassemble_the_same_frame(tmp_path):
    """bench.py's N > 1 path (rank -> bands, gather, row permutation) rehearsed with two ranks sharing the one GPU
    over gloo: the gathered 1920x1080 frame equals the single-rank frame bit for bit."""
    import subprocess
    import sys
    a, b = str(tmp_path / "one.pfm"), str(tmp_path / "two.pfm")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, os.path.join(scenes.ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--save-image", a],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    # the plain-shell form the driver uses for N = 1: bench.py starts the two ranks itself (vulkan_raytracing_amd/launcher.py)
    r = subprocess.run([sys.executable, os.path.join(scenes.ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline", "--rehearse-on-one-gpu", "--save-image", b], env={k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")},
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    import json
    assert json.loads(lines[0])["n_gpus"] == 2
    # ... and the launcher form of the contract (torch.distributed.run) gives the same frame
    c = str(tmp_path / "two_torchrun.pfm")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29517", os.path.join(scenes.ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--no-extras", "--rehearse-on-one-gpu", "--save-image", c], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(c, "rb").read() == open(b, "rb").read()
    fa, fb = open(a, "rb").read(), open(b, "rb").read()
    assert len(fa) == len(fb) and fa == fb
    # --gather-format rgba8: the ranks render the reference's 8-bit storage image (rt_set_param output_rgba8) and send 4 bytes per pixel —
    # the assembled frame is the binary32 frame quantised as the imageStore to an 8-bit image does (clamp, x 255, round)
    d = str(tmp_path / "two_rgba8.pfm")
    r = subprocess.run([sys.executable, os.path.join(scenes.ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--gather-format", "rgba8",
                        "--no-cpu-baseline", "--no-extras", "--rehearse-on-one-gpu", "--save-image", d], env={k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")},
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "rgba8" in json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][0])["config"]["gather_format"]
    import importlib.util
    spec = importlib.util.spec_from_file_location("image_diff", os.path.join(scenes.ROOT, "tools", "image_diff.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    f32, f8 = mod.read_image(a), mod.read_image(d)
    q = (np.clip(f32, 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
    assert np.array_equal(np.rint(f8 * 255.0).astype(np.uint8), q)


def test_bench_rccl_gather_path_single_rank(tmp_path):
    """The real RCCL code path of bench.py (process group on nccl, per-frame gather on the frame's stream, row
    permutation) with a world of one rank: must run and reproduce the plain frame."""
    import subprocess
    import sys
    a, b = str(tmp_path / "plain.pfm"), str(tmp_path / "coll.pfm")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for extra, out in (([], a), (["--force-collective"], b)):
        r = subprocess.run([sys.executable, os.path.join(scenes.ROOT, "bench.py"), "--steps", "6", "--warmup", "2", "--no-cpu-baseline", "--save-image", out] + extra,
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
    assert open(a, "rb").read() == open(b, "rb").read()


def test_headless_cpp_host_matches_python_path(tmp_path):
    """host/rt_headless.cpp (the reference's main() restated in C++ on the C ABI: ingest, BLAS/TLAS, per-frame
    animate -> TLAS refit -> uniforms -> trace, PFM output) renders the same frame as the ctypes path."""
    import subprocess
    exe = os.path.join(scenes.ROOT, "rt_headless")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-C", scenes.ROOT, "rt_headless"])
    out = str(tmp_path / "frame")
    W, H, frames, dt = 200, 120, 3, 0.5
    r = subprocess.run([exe, "--width", str(W), "--height", str(H), "--frames", str(frames), "--dt", str(dt), "--bounce", "3", "--spp", "2",
                        "--center", os.path.join(RES, "teapot.obj"), "--orbiting", os.path.join(RES, "cube.obj"),
                        "--skybox", os.path.join(RES, "skybox_texture_test"), "--out", out], cwd=scenes.ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    assert "Mrays/s" in r.stdout
    sys_path = os.path.join(scenes.ROOT, "tools")
    import importlib.util
    spec = importlib.util.spec_from_file_location("image_diff", os.path.join(sys_path, "image_diff.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    cpp = mod.read_image(out + ".pfm")
    # the same frame through Python: same scene, same fixed-step animation (timeParam += dt*0.1 per frame)
    ctx = RtContext(0)
    geom = host.SceneGeometry([os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj")])
    ctx.upload_geometry(geom.verts, geom.idx, geom.ranges)
    anim = host.SceneAnimation()
    ctx.set_instances(anim.instances((0, 1)))
    ctx.set_uniforms(host.default_uniforms(max_bounce_count=3, samples_per_pixel=2, orbiting_object_primitive_offset=geom.orbiting_primitive_offset,
                                           orbiting_object_vertex_offset=geom.orbiting_vertex_offset))
    ctx.set_skybox(host.load_skybox(os.path.join(RES, "skybox_texture_test")))
    tp = np.float32(0.0)
    for _ in range(frames):
        tp = np.float32(tp + np.float32(dt) * np.float32(0.1))
        anim.animate(float(tp))
        ctx.set_instances(anim.instances((0, 1)), update=True)
    img, _ = ctx.trace(W, H)
    ctx.close()
    assert np.array_equal(cpp, img[..., :3])
    ppm = mod.read_image(out + ".ppm")
    assert np.abs(ppm - np.clip(img[..., :3], 0, 1)).max() <= 0.5 / 255 + 1e-6


@pytest.mark.parametrize("algo", ["1", "2", "3"])
def test_device_built_blas_gives_identical_results(ctx, algo, monkeypatch):
    """rt_build_blas with blas_builder = 1 builds the BLAS on the GPU (csrc/bvh_gpu.hip: LBVH = algo 1, the default, or
    PLOC = algo 2).  Any valid BVH yields the same hits, so records and images must equal those of the host SAH builder
    and of the oracle."""
    monkeypatch.setenv("RT_GPU_BVH_ALGO", algo)
    arm, _ = host.armadillo_path(RES)
    rays = scenes.random_rays(30000, seed=77, target_radius=5.0)
    c2 = RtContext(0, variant="alt")      # (the quad kernel of the last step is in the alt build only)
    try:
        c2.set_param("blas_builder", 1)   # (the default)
        sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 2, 0, 3, 2, sky=scenes.synthetic_skybox(64), ctx=c2, time_param=0.4)
        g, st = c2.intersect(rays, counting=True)
        img, stf = c2.trace(256, 144)
        # the quad kernel needs the host-built BVH4: switching to it rebuilds the meshes on the host transparently
        c2.set_param("trace_variant", 1)
        g4, _ = c2.intersect(rays)
        assert np.array_equal(g, g4)
    finally:
        c2.close()
    c3 = RtContext(0)
    try:
        c3.set_param("blas_builder", 0)   # host binned-SAH
        sp_h = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 2, 0, 3, 2, sky=scenes.synthetic_skybox(64), ctx=c3, time_param=0.4)
        gh, sth = c3.intersect(rays, counting=True)
        imgh, _ = c3.trace(256, 144)
    finally:
        c3.close()
    assert np.array_equal(g, gh)
    assert np.array_equal(img, imgh)
    o = sp_h.orc.intersect(rays[:2000], use_bvh=True)
    assert np.array_equal(g[:2000]["prim"], o["prim"]) and np.array_equal(g[:2000]["t"].view(np.uint32), o["t"].view(np.uint32))
    # LBVH quality: more visits than SAH, but the same order of magnitude
    assert st.node_visits < 3 * sth.node_visits


def test_reference_default_bounce_budget_63(ctx):
    """The reference's own defaults: MAX_BOUNCE_COUNT 63 (include/config.h:26) with a refractive and a mirror object —
    exercises deep bounce queues, the host-side early exit of the per-bounce launches and the one-launch k_tail path."""
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 2, 1, 63, 2,
                                 sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.8)
    W, H = 160, 96
    ref, rc = sp.orc.render(W, H)
    imgs = {}
    try:
        # 0: one launch per bounce and kernel (with host polls), 2: bounces 1..63 inside one k_tail launch,
        # 1: the default (k_tail once a previous frame reported few secondary rays)
        for mode in (0, 2, 1):
            ctx.set_param("tail_kernel", mode)
            for _ in range(2):
                gpu, st = ctx.trace(W, H)
            assert_frame_equals_oracle(gpu, sp.orc, W, H, ref=ref)
            assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))
            imgs[mode] = (gpu, st.launches_total)
    finally:
        ctx.set_param("tail_kernel", 1)
    assert np.array_equal(imgs[0][0], imgs[2][0]) and np.array_equal(imgs[0][0], imgs[1][0])
    assert st.rays_secondary > st.rays_primary // 50


def test_general_affine_and_masked_instances(ctx):
    """Instance transforms with rotation about an arbitrary axis and NON-UNIFORM scale (normals need the inverse
    transpose, src/shader.rchit:94), plus an instance with mask 0 that must be invisible (ray mask 0xFF & 0 == 0)."""
    paths = [os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj")]

    def affine(axis, ang, scale, trans):
        a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        R = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)
        M = R @ np.diag(scale)
        return np.concatenate([M, np.asarray(trans, np.float64)[:, None]], axis=1).astype(np.float32).reshape(12)

    inst = np.zeros(4, scenes.INSTANCE_DTYPE)
    inst[0] = host.make_instance(affine((1, 2, 3), 0.7, (1.0, 0.5, 1.6), (-2.0, 0.5, 0.0)), 0, 0)
    inst[1] = host.make_instance(affine((0, 1, 1), -1.1, (2.0, 0.7, 0.9), (3.0, -1.0, 4.0)), 1, 1)
    inst[2] = host.make_instance(affine((1, 0, 0), 0.3, (1.5, 1.5, 0.4), (0.5, 2.5, 6.0)), 1, 0)
    hidden = host.make_instance(affine((0, 0, 1), 0.0, (6.0, 6.0, 6.0), (0.0, 0.0, 10.0)), 0, 1)
    hidden["custom_index_and_mask"] = 0 | (0x00 << 24)      # mask 0: a huge cube right in front of the camera, never hit
    inst[3] = hidden
    geom = host.SceneGeometry(paths)
    u = host.default_uniforms(max_bounce_count=3, samples_per_pixel=2, center_object_type=1, orbiting_object_type=0,
                              orbiting_object_primitive_offset=geom.orbiting_primitive_offset, orbiting_object_vertex_offset=geom.orbiting_vertex_offset)
    sp = scenes.ScenePair(paths, inst, u, sky=scenes.synthetic_skybox(64), ctx=ctx)
    W, H = 256, 144
    gpu, st = ctx.trace(W, H)
    ref, rc = sp.orc.render(W, H)
    assert_frame_equals_oracle(gpu, sp.orc, W, H, ref=ref)
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))
    rays = scenes.random_rays(5000, seed=5, target_radius=6.0)
    g, _ = ctx.intersect(rays)
    o = sp.orc.intersect(rays, use_bvh=False)
    assert np.array_equal(g, o) and not np.any(g["inst"] == 3) and np.any(g["inst"] == 2)


def test_mirrored_and_sheared_instances(ctx):
    """Instance transforms with negative determinant (a mirrored copy) and shear: hits are two-sided (instances are built
    with TRIANGLE_FACING_CULL_DISABLE, src/main.cpp:545-546) and normals go through the inverse transpose, so images and
    hit records must still equal the oracle's."""
    paths = [os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj")]
    mirror = np.array([[-1.2, 0.0, 0.0, -2.5], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.8, 1.0]], np.float32).reshape(12)
    shear = np.array([[1.0, 0.6, 0.0, 3.0], [0.0, 1.0, 0.3, -0.5], [0.2, 0.0, 1.0, 2.0]], np.float32).reshape(12)
    both = np.array([[0.0, -1.0, 0.4, 0.0], [1.5, 0.0, 0.0, 3.0], [0.0, 0.2, -0.7, 5.0]], np.float32).reshape(12)
    inst = np.zeros(3, scenes.INSTANCE_DTYPE)
    inst[0] = host.make_instance(mirror, 0, 0)
    inst[1] = host.make_instance(shear, 1, 1)
    inst[2] = host.make_instance(both, 1, 0)
    geom = host.SceneGeometry(paths)
    for ctype, otype in ((1, 0), (2, 1), (0, 2)):
        u = host.default_uniforms(max_bounce_count=4, samples_per_pixel=2, center_object_type=ctype, orbiting_object_type=otype,
                                  orbiting_object_primitive_offset=geom.orbiting_primitive_offset, orbiting_object_vertex_offset=geom.orbiting_vertex_offset)
        sp = scenes.ScenePair(paths, inst, u, sky=scenes.synthetic_skybox(64), ctx=ctx)
        W, H = 200, 112
        gpu, st = ctx.trace(W, H)
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(gpu, sp.orc, W, H, ref=ref)
        assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))
    rays = scenes.random_rays(5000, seed=11, target_radius=6.0)
    g, _ = ctx.intersect(rays)
    o = sp.orc.intersect(rays, use_bvh=False)
    assert np.array_equal(g, o) and len(np.unique(g["inst"])) == 4   # three instances and the misses


def test_cfg4_size_properties(ctx):
    """BASELINE config 4 size (3840x2160, depth 6): too big for the oracle, so size-independent properties only —
    determinism, alpha, ray bookkeeping, and 8 logical shards == the full frame bit for bit."""
    import torch
    arm, _ = host.armadillo_path(RES)
    scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 1, 0, 5, 4, sky=scenes.synthetic_skybox(128), ctx=ctx, time_param=1.3)
    W, H = 3840, 2160
    a, st = ctx.trace(W, H)
    assert st.rays_primary == W * H * 4 and st.rays_secondary > 0 and st.rays_shadow > 0
    assert np.all(a[..., 3] == 1.0) and np.isfinite(a).all()
    n = 8
    rows_max = tiling.max_shard_rows(H, tiling.BAND_ROWS, n)
    shards = []
    total = 0
    for s in range(n):
        buf = torch.zeros((rows_max, W, 4), dtype=torch.float32, device="cuda:0")
        ctx.trace_shard(W, H, tiling.BAND_ROWS, s, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
        stt = ctx.stats()
        total += stt.rays_primary + stt.rays_secondary + stt.rays_shadow
        torch.cuda.synchronize()
        shards.append(buf.cpu().numpy())
    assert np.array_equal(tiling.assemble(shards, H, W, tiling.BAND_ROWS), a)
    assert total == st.rays_primary + st.rays_secondary + st.rays_shadow


@pytest.mark.gpu
@pytest.mark.parametrize("n_tri", [8, 17, 33, 300])
def test_device_sah_builder_on_small_and_coincident_meshes(n_tri, tmp_path):
    """The level-by-level SAH builder (bvh_gpu.hip k_sah_*) at its seams: meshes around the 16-reference threshold between binned nodes
    and swept nodes, and a mesh whose triangles all share ONE centroid (no axis separates them: binned nodes fall back to position
    medians with the parent's box, swept nodes to halves) — hit records against the oracle's brute force."""
    rng = np.random.default_rng(100 + n_tri)
    for coincident in (False, True):
        if coincident:
            base = rng.normal(size=(3, 3))
            tris = np.stack([base * s for s in np.linspace(-1.0, 1.0, n_tri) if True])   # scaled copies about the origin: every centroid = the scaled base centroid
            tris = tris - tris.mean(axis=1, keepdims=True)                                 # ... moved to the origin: all centroids coincide
        else:
            tris = rng.normal(size=(n_tri, 3, 3))
        p = tmp_path / ("m%d_%d.obj" % (n_tri, int(coincident)))
        with open(p, "w") as f:
            for t in tris:
                for v in t:
                    f.write("v %.6f %.6f %.6f\nvn 0 0 1\n" % tuple(v))
            for i in range(len(tris)):
                f.write("f %d//%d %d//%d %d//%d\n" % (3 * i + 1, 3 * i + 1, 3 * i + 2, 3 * i + 2, 3 * i + 3, 3 * i + 3))
        c2 = RtContext(0)
        try:
            inst = [host.make_instance(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), 0, 0)]
            u = host.default_uniforms(max_bounce_count=1, samples_per_pixel=1, center_object_type=0, orbiting_object_type=0)
            sp = scenes.ScenePair([str(p)], inst, u, ctx=c2)
            rays = scenes.random_rays(6000, seed=5, origin_radius=6.0, target_radius=1.5)
            g, _ = c2.intersect(rays)
            o = sp.orc.intersect(rays, use_bvh=False)
            assert (o["inst"] >= 0).mean() > 0.05
            assert np.array_equal(g, o), (n_tri, coincident)
        finally:
            c2.close()


@pytest.mark.parametrize("algo", ["1", "2", "3"])
def test_device_builders_on_degenerate_soup(ctx, algo, monkeypatch, tmp_path):
    """Duplicate Morton codes, coincident and zero-area triangles, all triangles in one plane: the device builders must
    still produce a valid tree (checked against brute force through the oracle)."""
    monkeypatch.setenv("RT_GPU_BVH_ALGO", algo)
    rng = np.random.default_rng(11)
    pts = np.repeat(rng.normal(size=(40, 3)), 8, axis=0)          # 320 vertices, only 40 distinct positions
    pts[:80, 2] = 0.25                                            # a coplanar patch
    tri = rng.integers(0, len(pts), size=(700, 3))
    tri[:50] = tri[50:100]                                        # exact duplicates
    p = tmp_path / "soup.obj"
    with open(p, "w") as f:
        for v in pts:
            f.write("v %.6f %.6f %.6f\nvn 0 0 1\n" % tuple(v))
        for t in tri:
            f.write("f %d//%d %d//%d %d//%d\n" % (t[0] + 1, t[0] + 1, t[1] + 1, t[1] + 1, t[2] + 1, t[2] + 1))
    c2 = RtContext(0)
    try:
        inst = [host.make_instance(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), 0, 0)]
        u = host.default_uniforms(max_bounce_count=1, samples_per_pixel=1, center_object_type=0, orbiting_object_type=0)
        sp = scenes.ScenePair([str(p)], inst, u, ctx=c2)
        rays = scenes.random_rays(20000, seed=4, origin_radius=8.0, target_radius=2.5)
        g, _ = c2.intersect(rays)
        o = sp.orc.intersect(rays, use_bvh=False)
        assert (o["inst"] >= 0).mean() > 0.2
        assert np.array_equal(g, o)
        sh = rays.copy(); sh[:, 7] = 7.0
        ga, _ = c2.intersect(sh, any_hit=True)
        assert np.array_equal(ga["inst"] >= 0, sp.orc.intersect(sh, use_bvh=False)["inst"] >= 0)
    finally:
        c2.close()


# ---- BASELINE configurations on their real workloads (vulkan_raytracing_amd/workloads.py is what bench.py runs) ---------------
class _OracleTarget:
    """adapts the oracle scene to Workload.apply()"""

    def __init__(self):
        from oracle import oracle
        self.orc = oracle.OracleScene()

    def upload_geometry(self, verts, idx, ranges):
        self.orc.set_geometry(verts, idx, ranges)

    def set_instances(self, inst):
        self.orc.set_instances([inst[i].tobytes() for i in range(len(inst))])

    def set_uniforms(self, u):
        self.orc.set_uniforms(u.tobytes())

    def set_skybox(self, faces):
        self.orc.set_skybox(faces)


def _logical_shards_equal_full(ctx, W, H, n, full):
    import torch
    rows_max = tiling.max_shard_rows(H, tiling.BAND_ROWS, n)
    shards, total = [], 0
    for s in range(n):
        buf = torch.zeros((rows_max, W, 4), dtype=torch.float32, device="cuda:0")
        ctx.trace_shard(W, H, tiling.BAND_ROWS, s, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
        st = ctx.stats()
        total += st.rays_total
        torch.cuda.synchronize()
        shards.append(buf.cpu().numpy())
    assert np.array_equal(tiling.assemble(shards, H, W, tiling.BAND_ROWS), full)
    return total


@pytest.mark.parametrize("mesh", MESHES)
def test_cfg5_armadillo_x16_full_size(ctx, mesh):
    """BASELINE config 5 ON ITS WORKLOAD: 16 instances of the armadillo-class BLAS (stand-in, 345-348 k triangles) on a ring
    + the mirror teapot, 1920x1080, depth 4, spp 4 — exactly what `bench.py --workload cfg5` times.  Too big for a full
    oracle frame, so: determinism, alpha, ray bookkeeping with NON-ZERO bounce rays (the mirror teapot is in view and
    reflects the ring: the bounce rays walk the two-level BVH), 8 logical shards == the full frame bit for bit, and an
    oracle-rendered 8-row band through the teapot."""
    from vulkan_raytracing_amd import workloads
    wl = workloads.make("cfg5", RES, mesh=mesh)
    wl.apply(ctx)
    W, H = wl.width, wl.height
    assert (W, H) == (1920, 1080) and len(wl.instances) == 17 and int(wl.uniforms[0]["max_bounce_count"]) == 3
    a, st = ctx.trace(W, H)
    b, st2 = ctx.trace(W, H)
    assert np.array_equal(a, b)
    assert np.all(a[..., 3] == 1.0) and np.isfinite(a).all()
    assert st.rays_primary == W * H * 4 and st.rays_total == st2.rays_total
    assert st.rays_secondary > 10000, st.rays_secondary      # depth 4 is not vacuous: the teapot mirror is visible
    assert st.rays_shadow > W * H                            # the diffuse ring fills much of the frame
    assert _logical_shards_equal_full(ctx, W, H, 8, a) == st.rays_total
    tgt = _OracleTarget()
    wl.apply(tgt)
    # the band through the middle of the mirror teapot (bounce rays): project its centre (0, 0.8, 0) with src/shader.rgen:74-79
    u = wl.uniforms[0]
    rel = np.array([0.0, 0.8, 0.0]) - u["position"][:3]
    uy = 2.5 * float(rel @ u["up"][:3]) / float(rel @ u["forward"][:3])
    y0 = 8 * int(((1.0 - uy) * 0.5 * H) // 8)
    part, rc = tgt.orc.render(W, H, y0=y0, y1=y0 + 8)
    assert_frame_equals_oracle(a, tgt.orc, W, H, y0=y0, y1=y0 + 8, ref=part)
    assert int(rc[1]) > 0    # the oracle traced bounce rays in that band as well


def test_cfg2_full_size_real_skybox(ctx):
    """BASELINE config 2 ON ITS WORKLOAD: teapot (mirror) + cube, the real skybox_texture_test JPEG faces (2048^2, decoded by
    host/jpeg_decode.cpp), 1280x720, depth 2, spp 4 — the whole frame against the oracle."""
    from vulkan_raytracing_amd import workloads
    wl = workloads.make("cfg2", RES)
    wl.apply(ctx)
    assert wl.sky[0].shape == (2048, 2048, 4)
    W, H = wl.width, wl.height
    assert (W, H) == (1280, 720)
    gpu, st = ctx.trace(W, H)
    tgt = _OracleTarget()
    wl.apply(tgt)
    ref, rc = tgt.orc.render(W, H)
    assert_frame_equals_oracle(gpu, tgt.orc, W, H, ref=ref)
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))
    assert st.rays_secondary > 0 and st.rays_shadow > 0
    # most of the frame is sky: the real texture (flat labelled faces, few colours) must actually have been sampled
    assert len(np.unique(gpu[::8, ::8, :3].reshape(-1, 3), axis=0)) > 200


@pytest.mark.parametrize("mesh", MESHES)
def test_cfg3_reduced_size_real_sea_skybox(ctx, mesh):
    """BASELINE config 3 scene with its real skybox_texture_sea faces at 480x270 against the oracle (the full-size test
    above uses a synthetic cube map to keep the oracle band cheap)."""
    from vulkan_raytracing_amd import workloads
    wl = workloads.make("cfg3", RES, mesh=mesh)
    wl.apply(ctx)
    W, H = 480, 270
    gpu, st = ctx.trace(W, H)
    tgt = _OracleTarget()
    wl.apply(tgt)
    ref, rc = tgt.orc.render(W, H)
    assert_frame_equals_oracle(gpu, tgt.orc, W, H, ref=ref)
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))
    assert st.rays_secondary > 0 and st.rays_shadow > 0


def test_single_instance_scene_is_not_traversed_twice(ctx):
    """A one-instance TLAS has a synthetic root with one real child.  The absent child is an inverted box that no ray
    enters (it used to be a copy of its sibling, which made every ray walk the instance twice): node visits and triangle
    tests of the one-instance scene must not exceed those of the same scene plus a second, invisible instance."""
    cube = os.path.join(RES, "cube.obj")
    geom = host.SceneGeometry([cube])
    one = np.zeros(1, scenes.INSTANCE_DTYPE)
    one[0] = host.make_instance(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), 0, 0)
    two = np.zeros(2, scenes.INSTANCE_DTYPE)
    two[0] = one[0]
    far = host.make_instance(np.array([1, 0, 0, 500, 0, 1, 0, 500, 0, 0, 1, 500], np.float32), 0, 0)
    far["custom_index_and_mask"] = 0     # mask 0
    two[1] = far
    rays = scenes.random_rays(4096, seed=9, origin_radius=8.0, target_radius=1.0)
    ctx.upload_geometry(geom.verts, geom.idx, geom.ranges)
    ctx.set_uniforms(host.default_uniforms(max_bounce_count=0, samples_per_pixel=1))
    ctx.set_instances(one)
    g1, s1 = ctx.intersect(rays, counting=True)
    ctx.set_instances(two)
    g2, s2 = ctx.intersect(rays, counting=True)
    assert np.array_equal(g1, g2) and (g1["inst"] == 0).mean() > 0.5
    assert s1.tri_tests == s2.tri_tests and s1.node_visits <= s2.node_visits
    assert s1.tri_tests <= 12 * len(rays)


def test_tail_fault_falls_back_to_per_bounce_launches(ctx):
    """If a k_tail grid barrier gives up, the frame is rendered again with one launch per bounce and kernel instead of
    being discarded, and the context stays off k_tail (rt_stats.tail_faults counts it).  The fault is injected on the
    host side (rt_set_param debug_force_tail_fault): a real one needs another process squatting on the GPU."""
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 2, 1, 12, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.5)
    W, H = 160, 96
    c2 = RtContext(0)
    try:
        scenes.ScenePair(sp.geom_paths, sp.instances, sp.uniforms, sky=sp.sky, ctx=c2)
        c2.set_param("tail_kernel", 2)
        good, st0 = c2.trace(W, H)
        assert st0.tail_faults == 0
        c2.set_param("debug_force_tail_fault", 1)
        again, st1 = c2.trace(W, H)
        assert st1.tail_faults == 1 and np.array_equal(again, good)
        assert (st1.rays_primary, st1.rays_secondary, st1.rays_shadow) == (st0.rays_primary, st0.rays_secondary, st0.rays_shadow)
        c2.set_param("debug_force_tail_fault", 1)
        c2.trace_async(W, H)
        img, st2 = c2.trace_wait()
        assert np.array_equal(img, good) and st2.tail_faults == 1   # the context was already off k_tail: nothing to re-render
    finally:
        c2.close()


def test_hip_frames_match_the_reference_spirv_pixels(ctx):
    """The HIP path against tests/golden/spirv_fixtures.npz — pixels written by the reference's own shader.rgen.spv /
    shader.rchit.spv / miss modules under an interpreter (tests/golden/make_spirv_fixtures.py), at the BASELINE sizes
    (cfg1 256x256, cfg2 1280x720, cfg3 and cfg5 1920x1080 on both stand-in meshes).  Tolerance as in the CPU test of the
    oracle: 2e-4 on >= 99.5 % of the pixels (the kernels trace their own rays, 1 ulp off the recorded ones).  The recorded
    closest-hit rays go through rt_intersect as well: the hit records must be the recorded ones bit for bit."""
    for sc in scenes.load_spirv_fixtures():
        if sc.sky_dir is None:     # cfg1 has no cube map: a context that never had one (the module's context keeps its last)
            c1 = RtContext(0)
            try:
                sc.apply(c1)
                img, _ = c1.trace(sc.width, sc.height)
            finally:
                c1.close()
            px = sc.pixels
            d = np.abs(img[px["py"], px["px"]] - px["rgba"]).max(axis=1)
            assert (d <= 2e-4).mean() >= 0.995, (sc.name, float((d <= 2e-4).mean()), float(d.max()))
        sc.apply(ctx)
        img, _ = ctx.trace(sc.width, sc.height)
        px = sc.pixels
        got = img[px["py"], px["px"]]
        d = np.abs(got - px["rgba"]).max(axis=1)
        if sc.sky_dir is not None:
            assert (d <= 2e-4).mean() >= 0.995, (sc.name, float((d <= 2e-4).mean()), float(d.max()))
        b = sc.bounces
        rays = np.zeros((len(b), 8), np.float32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = b["o"], 0.001, b["d"], 10000.0
        g, _ = ctx.intersect(rays)
        assert np.array_equal(g["prim"], b["prim"]) and np.array_equal(g["inst"], b["inst"]), sc.name
        hit = b["inst"] >= 0
        for k in ("t", "u", "v"):
            assert np.array_equal(g[k][hit].view(np.uint32), b[k][hit].view(np.uint32)), (sc.name, k)
        sh = b["shadow"] == 1
        srays = np.zeros((int(sh.sum()), 8), np.float32)
        srays[:, 0:3], srays[:, 3], srays[:, 4:7], srays[:, 7] = b["so"][sh], 0.001, b["sl"][sh], b["stmax"][sh]
        ga, _ = ctx.intersect(srays, any_hit=True)
        assert np.array_equal(ga["inst"] >= 0, b["occluded"][sh] == 1), sc.name


def test_frame_slots_share_one_scene(ctx):
    """rt_create_frame_slot: three more frames in flight on ONE scene (geometry, BLAS, cube map uploaded once), each slot with
    its own instance transforms (a different moment of the animation), uniforms, queues and stream.  Every slot's frame must
    equal the frame of a stand-alone context given the same inputs; scene-building calls on any member invalidate every
    slot's TLAS; a new cube map on the root is what the slots sample next."""
    import torch
    paths = (os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"))
    W, H = 200, 120
    root = RtContext(0)
    slots = []
    try:
        sp = scenes.two_object_scene(paths[0], paths[1], 1, 0, 3, 2, sky=scenes.synthetic_skybox(64), ctx=root)
        sp.ctx = None                                    # from here on `sp` drives the oracle only

        def oracle_frame(instances, max_bounce, img=None, ref=None):
            """the oracle's frame for these instances and bounce budget; with img: asserts that img equals it (ref: that frame, rendered before)"""
            u = sp.uniforms.copy()
            u[0]["max_bounce_count"] = max_bounce
            sp.set_instances(instances)
            sp.orc.set_uniforms(u.tobytes())
            if img is None:
                return sp.orc.render(W, H)[0]
            return assert_frame_equals_oracle(img, sp.orc, W, H, ref=ref)

        slots = [root] + [root.frame_slot() for _ in range(3)]
        anim = host.SceneAnimation()
        inst, want = [], []
        for k, c in enumerate(slots):
            anim.animate(0.15 * (k + 1))
            inst.append(anim.instances((0, 1)))
            u = sp.uniforms.copy()
            u[0]["max_bounce_count"] = 1 + k            # per-slot uniform block
            c.set_instances(inst[k])
            c.set_uniforms(u)
            want.append(oracle_frame(inst[k], 1 + k))
        for _ in range(2):                               # all four in flight at once, twice
            for c in slots:
                c.trace_async(W, H)
            for k, c in enumerate(slots):
                img, st = c.trace_wait()
                oracle_frame(inst[k], 1 + k, img, ref=want[k])
        # refit on one slot while the others have frames pending: only that slot's frame is waited for
        for c in slots[1:]:
            c.trace_async(W, H)
        anim.animate(0.9)
        moved = anim.instances((0, 1))
        slots[0].set_instances(moved, update=True)
        img0, _ = slots[0].trace(W, H)
        oracle_frame(moved, 1, img0)
        for k, c in enumerate(slots[1:], 1):
            img, _ = c.trace_wait()
            oracle_frame(inst[k], 1 + k, img, ref=want[k])
        # a frame on a caller's stream right behind a refit (the upload travels on the context's own stream)
        buf = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        s2 = torch.cuda.Stream()
        slots[2].set_instances(moved, update=True)
        slots[2].trace_shard(W, H, H, 0, 1, buf.data_ptr(), buf.numel() * 4, s2.cuda_stream)
        slots[2].synchronize()
        oracle_frame(moved, 3, buf.cpu().numpy())
        # the cube map is shared: replacing it through the root changes what every slot samples
        sky2 = scenes.synthetic_skybox(32, seed=99)
        root.set_skybox(sky2)
        sp.orc.set_skybox(sky2)
        img, _ = slots[3].trace(W, H)
        oracle_frame(inst[3], 4, img)
        # scene-building on any member: every slot has to set its instances again
        slots[1].upload_geometry(sp.geom.verts, sp.geom.idx, sp.geom.ranges)
        for c in slots:
            with pytest.raises(RtError) as e:
                c.trace(W, H)
            assert e.value.code == 2
        slots[3].set_instances(inst[3])
        img, _ = slots[3].trace(W, H)
        oracle_frame(inst[3], 4, img)
        with pytest.raises(RtError):
            [root.frame_slot() for _ in range(16)]       # at most 16 contexts per scene
    finally:
        for c in reversed(slots[1:]):
            c.close()
        root.close()


def test_headless_multi_gpu_host_rccl_and_logical_shards(tmp_path):
    """host/rt_headless --gpus N (librt_multi.so: one C++ process, band sharding, ONE gather per frame, de-interleave on the
    root) against the single-context path of the same program: (a) N = 4 LOGICAL devices on this one GPU with the shards
    moved by device copies (--loopback), (b) N = 1 through real RCCL (ncclCommInitAll + ncclGather on the frame's stream).
    Same animated frame sequence, two frames in flight everywhere: the last frame must be identical bit for bit, in RGBA32F
    and in the 8-bit surface format."""
    import importlib.util
    import subprocess
    exe = os.path.join(scenes.ROOT, "rt_headless")
    spec = importlib.util.spec_from_file_location("image_diff", os.path.join(scenes.ROOT, "tools", "image_diff.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    common = ["--width", "328", "--height", "203", "--frames", "5", "--dt", "0.5", "--bounce", "3", "--spp", "2", "--frames-in-flight", "2",
              "--center", os.path.join(RES, "teapot.obj"), "--orbiting", os.path.join(RES, "cube.obj"), "--skybox", os.path.join(RES, "skybox_texture_test")]
    outs = {}
    for name, extra in (("single", []), ("loop4", ["--gpus", "4", "--loopback"]), ("rccl1", ["--gpus", "1"]), ("loop3", ["--gpus", "3", "--loopback"]),
                        ("loop3_passes", ["--gpus", "3", "--loopback", "--batch", "3"]), ("rccl1_passes", ["--gpus", "1", "--batch", "4"])):
        out = str(tmp_path / name)
        r = subprocess.run([exe] + common + extra + ["--out", out], cwd=scenes.ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, name + ": " + r.stdout[-800:] + r.stderr[-1500:]
        assert "Mrays/s" in r.stdout
        outs[name] = mod.read_image(out + ".pfm")
    assert outs["single"].shape == (203, 328, 3) and np.isfinite(outs["single"]).all() and outs["single"].std() > 0.01
    for name in ("loop4", "rccl1", "loop3", "loop3_passes", "rccl1_passes"):     # (…_passes: rtm_set_batch, several frames per pass, one gather per pass)
        assert np.array_equal(outs[name], outs["single"]), name
    pp = {}
    for name, extra in (("single8", ["--rgba8"]), ("loop4_8", ["--gpus", "4", "--loopback", "--rgba8"])):
        out = str(tmp_path / name)
        r = subprocess.run([exe] + common + extra + ["--out", out], cwd=scenes.ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, name + ": " + r.stdout[-800:] + r.stderr[-1500:]
        pp[name] = open(out + ".ppm", "rb").read()
    assert pp["single8"] == pp["loop4_8"]


def test_cube_seams_and_corners_on_the_gpu(ctx):
    """Frames whose sky lookups straddle cube edges and a cube corner: an 8x8-texel cube map (half a texel is several degrees
    wide) seen by a camera turned towards the +X/+Z/+Y corner.  sample_sky's neighbour-face taps and corner rule against
    the oracle's, which tests/test_oracle.py checks against an independent float64 sampler and for continuity."""
    rng = np.random.default_rng(17)
    faces = []
    for f in range(6):
        img = np.zeros((8, 8, 4), np.uint8)
        img[..., :3] = rng.integers(0, 256, (8, 8, 3))
        img[..., 3] = 255
        faces.append(img)
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 1, 0, 2, 2, sky=faces, ctx=ctx)
    W, H = 320, 200
    seen = 0
    for yaw, pitch in ((0.0, 0.0), (np.pi / 4, 0.0), (np.pi / 4, 0.6155), (-2.2, -0.62), (3.0, 1.2)):
        cam = host.Camera((0.0, 0.0, 20.0))
        cam.process_mouse_movement(float(yaw), float(pitch))
        u = sp.uniforms.copy()
        cam.to_uniforms(u)
        sp.set_uniforms(u)
        gpu, st = ctx.trace(W, H)
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(gpu, sp.orc, W, H, ref=ref)
        assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))
        seen += 1
    assert seen == 5


def test_row_n4_mtl_materials_and_instance_types(ctx):
    """SURVEY.md §8(f) n4 on the HIP path: (a) cube_scene.obj shaded with the 8 materials of its own cube_scene.mtl (per-face
    usemtl -> Ka/Kd/Ks/Ns per triangle); (b) five instances with per-instance types (diffuse / mirror / refractive) instead of
    the reference's two-way switch, materials with their own Ni and an illum-style forced type — all against the oracle;
    (c) removing table and types gives the reference's frame again, bit for bit."""
    from vulkan_raytracing_amd.api import MATERIAL_TYPE_OF_INSTANCE
    c2 = RtContext(0, variant="alt")      # (step (b) also runs the alternative traversal kernels, which the product library does not hold)
    try:
        inst = [host.make_instance(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), 0, 0)]
        u = host.default_uniforms(max_bounce_count=2, samples_per_pixel=2, center_object_type=0, orbiting_object_type=0)
        sp = scenes.ScenePair([os.path.join(RES, "cube_scene.obj")], inst, u, sky=scenes.synthetic_skybox(64), ctx=c2)
        W, H = 256, 256
        base, _ = c2.trace(W, H)
        g = sp.geom
        assert len(g.materials) == 9
        sp.set_materials(g.materials, g.prim_material)
        gpu, st = c2.trace(W, H)
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(gpu, sp.orc, W, H, ref=ref)
        assert np.abs(gpu - base).max() > 0.05 and (st.rays_primary, st.rays_secondary, st.rays_shadow) == tuple(int(x) for x in rc)
        # (b) teapot + cube meshes, five instances, types per instance, a glass material with Ni 1.2 and a forced-mirror material
        paths = [os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj")]
        inst5 = np.zeros(5, scenes.INSTANCE_DTYPE)
        place = [((0, 0, 0), 0, 0), ((-4.5, 0, 2), 1, 1), ((4.5, 0.5, 2), 1, 1), ((0, -3.5, 3), 1, 1), ((0, 3.5, 1), 1, 0)]
        for k, (t, ci, mesh) in enumerate(place):
            inst5[k] = host.make_instance(np.array([1, 0, 0, t[0], 0, 1, 0, t[1], 0, 0, 1, t[2]], np.float32), ci, mesh)
        geom = host.SceneGeometry(paths)
        u5 = host.default_uniforms(max_bounce_count=4, samples_per_pixel=2, center_object_type=1, orbiting_object_type=0,
                                   orbiting_object_primitive_offset=geom.orbiting_primitive_offset, orbiting_object_vertex_offset=geom.orbiting_vertex_offset)
        sp5 = scenes.ScenePair(paths, inst5, u5, sky=scenes.synthetic_skybox(64), ctx=c2)
        before, _ = c2.trace(320, 200)
        tbl = sp5.geom.materials.copy()                     # 0 = reference surface, 1 = teapot.mtl, 2 = cube.mtl (if any)
        assert len(tbl) >= 2
        tbl["kd"][1] = (0.9, 0.3, 0.1); tbl["ns"][1] = 37.0; tbl["ni"][1] = 1.2; tbl["ka"][1] = (0.2, 0.1, 0.05)
        pm = sp5.geom.prim_material.copy()
        # the cube's bottom half of triangles becomes a forced mirror (as `illum 3` would), the rest the reference surface
        cube_first = sp5.geom.ranges[1][1] // 3
        forced = np.zeros(1, tbl.dtype); forced[0] = tbl[0]; forced["type"] = 1
        tbl = np.concatenate([tbl, forced])
        pm[cube_first:cube_first + 6] = len(tbl) - 1
        pm[cube_first + 6:] = 0
        sp5.set_materials(tbl, pm)
        sp5.set_instance_types([2, 0, 1, 2, 0])
        gpu5, st5 = c2.trace(320, 200)
        ref5, rc5 = sp5.orc.render(320, 200)
        assert_frame_equals_oracle(gpu5, sp5.orc, 320, 200, ref=ref5)
        assert (st5.rays_primary, st5.rays_secondary, st5.rays_shadow) == tuple(int(x) for x in rc5)
        assert np.abs(gpu5 - before).max() > 0.05 and st5.rays_secondary > 0 and st5.rays_shadow > 0
        # the other traversal variants shade through the same code
        for v in (2, 1):
            c2.set_param("trace_variant", v)
            img, _ = c2.trace(320, 200)
            assert np.array_equal(img, gpu5), v
        c2.set_param("trace_variant", 0)
        # (c) back to the reference
        sp5.set_materials(None)
        sp5.set_instance_types(None)
        after, _ = c2.trace(320, 200)
        assert np.array_equal(after, before)
        with pytest.raises(RtError):
            c2.set_materials(tbl, pm[:-1])                  # one id per triangle of the index buffer
        with pytest.raises(RtError):
            c2.set_instance_types([0, 3])
    finally:
        c2.close()



@pytest.mark.parametrize("name,mesh", [("cfg3", "standin"), ("cfg3", "limbs"), ("cfg4", "standin"), ("cfg5", "standin")])
def test_baseline_workloads_whole_frame_at_full_size_against_the_oracle(ctx, name, mesh):
    """The BASELINE configurations bench.py times, at their FULL size, every pixel against the oracle: cfg3 (1920x1080,
    depth 4, real sea skybox) on both stand-in meshes, cfg4 (3840x2160, depth 6), cfg5 (16 instances, raised camera).
    The oracle renders them on the GPU box's host cores (its own SAH BVH, all threads): 10-40 M rays each, a second or
    two.  Bar: bit-identical on >= 99.9 % of the pixels, identical ray counts."""
    import time
    from vulkan_raytracing_amd import workloads
    wl = workloads.make(name, RES, mesh=mesh)
    wl.apply(ctx)
    W, H = wl.width, wl.height
    gpu, st = ctx.trace(W, H)
    tgt = _OracleTarget()
    wl.apply(tgt)
    t0 = time.time()
    ref, rc = tgt.orc.render(W, H)
    print("oracle %s/%s: %.1f s for %d rays" % (name, mesh, time.time() - t0, int(rc.sum())))
    assert_frame_equals_oracle(gpu, tgt.orc, W, H, ref=ref)
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))
    assert st.rays_primary == W * H * 4 and st.rays_secondary > 0 and st.rays_shadow > 0


def test_animated_cfg3_frames_at_full_size_against_the_oracle(ctx):
    """bench.py's animated leg on its workload: cfg3 after 20 and 90 steps of the reference's animation
    (src/main.cpp:2836-2851, fixed dt), each through rt_set_instances(update=1) = TLAS refit, whole 1920x1080 frames
    against the oracle (which rebuilds its TLAS)."""
    from vulkan_raytracing_amd import workloads
    wl = workloads.make("cfg3", RES)
    wl.apply(ctx)
    tgt = _OracleTarget()
    wl.apply(tgt)
    W, H = wl.width, wl.height
    ctx.trace(W, H)
    t = np.float32(0.0)
    for step in range(1, 91):
        t = np.float32(t + np.float32(1.0 / 60.0) * np.float32(0.1))
        inst = wl.animate(t)
        if step in (20, 90):
            ctx.set_instances(inst, update=True)
            gpu, st = ctx.trace(W, H)
            tgt.set_instances(inst)
            ref, rc = tgt.orc.render(W, H)
            assert_frame_equals_oracle(gpu, tgt.orc, W, H, ref=ref)
            assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))


def test_grazing_rays_against_brute_force(ctx):
    """Rays almost parallel to a coordinate plane that skim the axis-aligned faces of cube.obj (every box face of its tree
    carries triangles) and the teapot: hit records of the HIP traversal (quantized boxes, slack in space) against the
    oracle's BRUTE-FORCE mode, closest hit and any hit; and a TLAS whose instances are rotated so that the instance boxes
    are grazed as well."""
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 1, 0, 1, 1, ctx=ctx)
    rays = scenes.grazing_rays(60000, seed=11)
    g, _ = ctx.intersect(rays)
    b = sp.orc.intersect(rays, use_bvh=False)
    assert (b["inst"] >= 0).mean() > 0.2
    same = (g["prim"] == b["prim"]) & (g["inst"] == b["inst"]) & (g["t"].view(np.uint32) == b["t"].view(np.uint32))
    assert same.all(), int((~same).sum())
    sh = rays.copy(); sh[:, 7] = 21.0
    ga, _ = ctx.intersect(sh, any_hit=True)
    clo = sp.orc.intersect(sh, use_bvh=False)
    assert np.array_equal(ga["inst"] >= 0, clo["inst"] >= 0)
    sp2 = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 1, 0, 1, 1, ctx=ctx, time_param=0.25)
    g2, _ = ctx.intersect(rays)
    b2 = sp2.orc.intersect(rays, use_bvh=False)
    same2 = (g2["prim"] == b2["prim"]) & (g2["inst"] == b2["inst"]) & (g2["t"].view(np.uint32) == b2["t"].view(np.uint32))
    assert same2.all(), int((~same2).sum())


def test_degenerate_frames_and_empty_shards(ctx):
    """Edge cases of the dispatch (src/main.cpp:2620-2624 with unusual extents): a 1x1 frame, frames smaller than one 8x8
    tile, more shards than bands (some ranks render NOTHING and must leave their buffers and counters alone), a camera that
    looks away from every object (every sample ends in k_raygen), maxBounceCount 0."""
    import torch
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 1, 0, 2, 3, sky=scenes.synthetic_skybox(64), ctx=ctx)
    for W, H in ((1, 1), (3, 2), (7, 9), (64, 1)):
        gpu, st = ctx.trace(W, H)
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(gpu, sp.orc, W, H, ref=ref)
        assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))
    # 5 shards over a frame of two 8-row bands: shards 2, 3, 4 are empty
    W, H, n = 96, 16, 5
    full, st = ctx.trace(W, H)
    rows_max = tiling.max_shard_rows(H, tiling.BAND_ROWS, n)
    shards, total = [], 0
    for s in range(n):
        buf = torch.full((max(rows_max, 1), W, 4), -7.0, dtype=torch.float32, device="cuda:0")
        ctx.trace_shard(W, H, tiling.BAND_ROWS, s, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
        stt = ctx.stats()
        rows = ctx.shard_rows(H, tiling.BAND_ROWS, s, n)
        assert rows == (8 if s < 2 else 0)
        if rows == 0:
            assert (stt.rays_primary, stt.rays_secondary, stt.rays_shadow) == (0, 0, 0)
            assert bool((buf == -7.0).all())           # an empty shard writes nothing
        total += stt.rays_primary + stt.rays_secondary + stt.rays_shadow
        shards.append(buf.cpu().numpy()[:rows_max])
    assert np.array_equal(tiling.assemble(shards, H, W, tiling.BAND_ROWS), full)
    assert total == st.rays_primary + st.rays_secondary + st.rays_shadow
    # a frame right after the empty ones is still correct (counter blocks ping-pong untouched)
    again, _ = ctx.trace(W, H)
    assert np.array_equal(again, full)
    # camera turned away from both objects: only sky
    u = sp.uniforms.copy()
    u[0]["forward"][:3] = (0.0, 0.0, 1.0)
    sp.set_uniforms(u)
    gpu, st = ctx.trace(160, 90)
    ref, rc = sp.orc.render(160, 90)
    assert_frame_equals_oracle(gpu, sp.orc, 160, 90, ref=ref)
    assert st.rays_secondary == 0 and st.rays_shadow == 0 and int(rc[1]) == 0 and int(rc[2]) == 0
    # maxBounceCount 0: primary rays and their shadow rays only
    u = sp.uniforms.copy()
    u[0]["forward"][:3] = (0.0, 0.0, -1.0)
    u[0]["max_bounce_count"] = 0
    sp.set_uniforms(u)
    gpu, st = ctx.trace(160, 90)
    ref, rc = sp.orc.render(160, 90)
    assert_frame_equals_oracle(gpu, sp.orc, 160, 90, ref=ref)
    assert st.rays_secondary == 0 and (st.rays_primary, st.rays_shadow) == (int(rc[0]), int(rc[2]))


def test_more_instances_than_the_lds_record_cache(ctx):
    """k_trace stages the records of the first 32 instances in LDS and reads the others from global memory: 48 cubes on a
    ring + the mirror teapot (49 instances, a 6-level TLAS), whole frame and hit records against the oracle, then the
    same TLAS refitted after every instance moved."""
    from vulkan_raytracing_amd import workloads
    paths = [os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj")]
    g = host.SceneGeometry(paths)
    u = host.default_uniforms(max_bounce_count=2, samples_per_pixel=2, center_object_type=1, orbiting_object_type=0,
                              orbiting_object_primitive_offset=g.orbiting_primitive_offset, orbiting_object_vertex_offset=g.orbiting_vertex_offset)
    workloads.raised_camera(u)
    inst = workloads.ring_instances(48, 12.0)
    sp = scenes.ScenePair(paths, inst, u, sky=scenes.synthetic_skybox(64), ctx=ctx)
    W, H = 320, 180
    gpu, st = ctx.trace(W, H)
    ref, rc = sp.orc.render(W, H)
    assert_frame_equals_oracle(gpu, sp.orc, W, H, ref=ref)
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))
    assert st.rays_secondary > 0 and st.rays_shadow > 0
    rays = scenes.random_rays(30000, seed=9, origin_radius=30.0, target_radius=13.0)
    gh, _ = ctx.intersect(rays)
    oh = sp.orc.intersect(rays, use_bvh=False)
    assert len(np.unique(oh["inst"][oh["inst"] >= 0])) > 40      # the rays reach instances beyond the first 32
    same = (gh["prim"] == oh["prim"]) & (gh["inst"] == oh["inst"]) & (gh["t"].view(np.uint32) == oh["t"].view(np.uint32))
    assert same.all(), int((~same).sum())
    sp.set_instances(workloads.ring_instances(48, 12.0, phase=0.37), update=True)
    gpu2, st2 = ctx.trace(W, H)
    ref2, rc2 = sp.orc.render(W, H)
    assert_frame_equals_oracle(gpu2, sp.orc, W, H, ref=ref2)
    assert (st2.rays_primary, st2.rays_secondary, st2.rays_shadow) == (int(rc2[0]), int(rc2[1]), int(rc2[2]))


def test_primary_ray_coverage_mask_is_result_identical(ctx):
    """k_cover marks the 8x8-pixel tiles the meshes' frontier boxes project onto and k_raygen shades the samples of the other
    tiles as misses without any box test (rt_set_param "primary_cover", default on).  It may only remove rays that would have
    missed: frames and ray counts with the mask on and off are identical — ordinary camera, a camera INSIDE an instance's box
    (a frontier box crosses the camera plane: everything marked), a sheared / non-unit camera basis, objects partly off
    screen, band shards of 8 and 16 rows (mask on) and 5 rows (mask off) — fewer rays reach the traversal kernel, and the
    frame equals the oracle's."""
    import torch
    arm, _ = host.armadillo_path(RES)
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 1, 0, 2, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.45)
    W, H = 408, 232

    def both():
        out = {}
        for on in (1, 0):
            ctx.set_param("primary_cover", on)
            img, st = ctx.trace(W, H)
            out[on] = (img, (st.rays_primary, st.rays_secondary, st.rays_shadow), st.closest_rays)
        ctx.set_param("primary_cover", 1)
        assert np.array_equal(out[1][0], out[0][0]) and out[1][1] == out[0][1]
        return out

    base_u = sp.uniforms.copy()
    try:
        out = both()
        assert out[1][2] < 0.8 * out[0][2], (out[1][2], out[0][2])      # the mask removes rays that the instance boxes let through
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(out[1][0], sp.orc, W, H, ref=ref)
        assert out[1][1] == (int(rc[0]), int(rc[1]), int(rc[2]))
        # shards: 8- and 16-row bands use the mask, 5-row bands cannot (tiles would straddle bands)
        for band, n in ((8, 3), (16, 2), (5, 3)):
            rows_max = tiling.max_shard_rows(H, band, n)
            shards = []
            for s in range(n):
                buf = torch.zeros((rows_max, W, 4), dtype=torch.float32, device="cuda:0")
                ctx.trace_shard(W, H, band, s, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
                ctx.synchronize()
                shards.append(buf.cpu().numpy())
            assert np.array_equal(tiling.assemble(shards, H, W, band), out[1][0])
        # camera inside the orbiting mesh's bounding box, looking at the teapot
        u = base_u.copy()
        u[0]["position"][:3] = (0.3, 0.2, 5.2)
        sp.set_uniforms(u); both()
        # sheared, non-unit basis (the shader takes the vectors as they come, src/shader.rgen:74-79)
        u = base_u.copy()
        u[0]["right"][:3] = (1.3, 0.2, 0.1); u[0]["up"][:3] = (0.15, 0.8, -0.1); u[0]["forward"][:3] = (0.1, -0.05, -1.4)
        sp.set_uniforms(u); o2 = both()
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(o2[1][0], sp.orc, W, H, ref=ref)
        # objects partly off screen, and behind the camera
        u = base_u.copy()
        u[0]["position"][:3] = (3.5, 0.5, 9.0)
        sp.set_uniforms(u); both()
        u = base_u.copy()
        u[0]["forward"][:3] = (0.0, 0.0, 1.0)
        sp.set_uniforms(u); o3 = both()
        assert o3[1][2] == 0 and o3[0][2] == 0
    finally:
        ctx.set_param("primary_cover", 1)
        sp.set_uniforms(base_u)


def test_entry_points_are_result_identical(ctx):
    """k_entry gives every covered 8x8-pixel tile a short list of deep subtrees (its beam against the TLAS and the nearest
    instance's BLAS) and the primary rays of the tile start their walk there instead of at the TLAS root (rt_set_param
    "entry_points", default on).  The list must contain everything a ray of the tile can hit: frames, ray counts and the
    number of rays that reach the traversal kernel are identical with it on and off or it removed a hit; the frame equals the
    oracle's; node visits per ray drop.  Cameras: the start-up one, inside an instance's box, a sheared basis, objects partly
    off screen / behind the camera; band shards; 17 instances (more TLAS words than a record holds); a one-instance scene."""
    import torch
    arm, _ = host.armadillo_path(RES)
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 1, 0, 2, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.45)
    W, H = 408, 232

    def both(w=W, h=H):
        out = {}
        for on in (1, 0):
            ctx.set_param("entry_points", on)
            img, st = ctx.trace(w, h, counting=True)
            out[on] = (img, (st.rays_primary, st.rays_secondary, st.rays_shadow), st.closest_rays, st.node_visits)
        ctx.set_param("entry_points", 1)
        assert np.array_equal(out[1][0], out[0][0]) and out[1][1] == out[0][1]
        assert out[1][2] <= out[0][2]          # empty tiles only remove rays
        return out

    base_u = sp.uniforms.copy()
    try:
        out = both()
        assert out[1][3] < 0.9 * out[0][3], (out[1][3], out[0][3])      # fewer node visits for the same result (pixels this coarse, two samples: the pixel beams' walks are wide)
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(out[1][0], sp.orc, W, H, ref=ref)
        assert out[1][1] == (int(rc[0]), int(rc[1]), int(rc[2]))
        for band, n in ((8, 3), (16, 2)):
            rows_max = tiling.max_shard_rows(H, band, n)
            shards = []
            for s in range(n):
                buf = torch.zeros((rows_max, W, 4), dtype=torch.float32, device="cuda:0")
                ctx.trace_shard(W, H, band, s, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
                ctx.synchronize()
                shards.append(buf.cpu().numpy())
            assert np.array_equal(tiling.assemble(shards, H, W, band), out[1][0])
        u = base_u.copy()
        u[0]["position"][:3] = (0.3, 0.2, 5.2)            # inside the orbiting mesh's box
        sp.set_uniforms(u); both()
        u = base_u.copy()
        u[0]["right"][:3] = (1.3, 0.2, 0.1); u[0]["up"][:3] = (0.15, 0.8, -0.1); u[0]["forward"][:3] = (0.1, -0.05, -1.4)
        sp.set_uniforms(u); o2 = both()
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(o2[1][0], sp.orc, W, H, ref=ref)
        u = base_u.copy()
        u[0]["position"][:3] = (3.5, 0.5, 9.0)            # partly off screen, very close
        sp.set_uniforms(u); both()
        u = base_u.copy()
        u[0]["position"][:3] = (0.0, 0.0, 2000.0)         # far away: the whole scene inside a few tiles
        sp.set_uniforms(u); both()
        u = base_u.copy()
        u[0]["forward"][:3] = (0.0, 0.0, 1.0)             # everything behind the camera
        sp.set_uniforms(u); both()
        # refractive centre mesh + deeper bounce budget: later bounces must be unaffected
        u = base_u.copy()
        u[0]["center_object_type"] = 2; u[0]["max_bounce_count"] = 5
        sp.set_uniforms(u); both()
    finally:
        ctx.set_param("entry_points", 1)
        sp.set_uniforms(base_u)
    # 17 instances: the beam of a tile can meet more instances than a record has TLAS words
    wl = workloads.make("cfg5", RES)
    wl.apply(ctx, sky=scenes.synthetic_skybox(64))
    ctx.set_param("entry_max_instances", 64)      # (the default is 32)
    try:
        o5 = both(480, 270)
    finally:
        ctx.set_param("entry_max_instances", 32)
    assert o5[1][3] < o5[0][3]
    # a single instance (synthetic TLAS root with an absent child) and a single-triangle-leaf mesh
    wl1 = workloads.make("cfg1", RES)
    wl1.apply(ctx)
    both(256, 256)


def test_frame_batches_equal_the_frames_rendered_one_by_one(ctx):
    """rt_set_batch + rt_trace_shard_batch send K consecutive frames through ONE pass of the pipeline (the bands of a
    rank of an N-GPU split are then launches of whole-frame size again).  Every frame has its own instances (a TLAS refit each, as
    src/main.cpp:2848-2861 does per frame), camera and light; instance ids, TLAS roots and sample ids are per frame inside the kernels.
    The K images and the summed ray counts must equal those of the K frames rendered one after another, bit for bit: whole frames and
    band shards, an animated sequence with a moving camera and light, K = 1 .. 8, mirror and glass bounces (k_tail over all frames),
    17 instances; and one frame of the batch equals the oracle's."""
    import torch
    from vulkan_raytracing_amd.api import INSTANCE_DTYPE, UNIFORMS_DTYPE
    arm, _ = host.armadillo_path(RES)
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 1, 0, 3, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.2)
    W, H = 264, 152
    anim = host.SceneAnimation()

    def frame_inputs(k):
        anim2 = host.SceneAnimation()
        for j in range(k + 1):
            anim2.animate(np.float32(0.2 + 0.07 * (j + 1)))
        inst = anim2.instances((0, 1))
        u = sp.uniforms.copy()
        u[0]["position"][:3] = (0.4 * k - 1.0, 0.2 * k, 20.0 - 0.8 * k)
        u[0]["light_position"][:3] = (5.0 - k, 5.0 + 0.5 * k, 5.0); u[0]["light_intensity"] = 0.5 + 0.25 * k
        return np.ascontiguousarray(inst, INSTANCE_DTYPE), u

    def one_by_one(frames, band, shard, n):
        rows = tiling.max_shard_rows(H, band, n)
        imgs, rays = [], np.zeros(3, np.int64)
        first = True
        for inst, u in frames:
            ctx.set_instances(inst, update=not first); first = False
            ctx.set_uniforms(u)
            buf = torch.zeros((rows, W, 4), dtype=torch.float32, device="cuda:0")
            ctx.trace_shard(W, H, band, shard, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
            st = ctx.stats()
            rays += (st.rays_primary, st.rays_secondary, st.rays_shadow)
            imgs.append(buf.cpu().numpy())
        return imgs, rays

    def batched(frames, band, shard, n, update):
        rows = tiling.max_shard_rows(H, band, n)
        K = len(frames)
        ctx.set_batch(np.stack([f[0] for f in frames]), np.concatenate([f[1] for f in frames]), update=update)
        buf = torch.zeros((K, rows, W, 4), dtype=torch.float32, device="cuda:0")
        rows_real = ctx.shard_rows(H, band, shard, n)
        padded = (K + band + shard) % 2 == 1       # frame k's shard rows_max rows behind frame k - 1's (a padded buffer), or back to back
        ctx.trace_shard_batch(W, H, band, shard, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream,
                              frame_stride_bytes=rows * W * 16 if padded else 0)
        st = ctx.stats()
        out = buf.cpu().numpy()
        imgs = []
        for k in range(K):
            flat = out.reshape(-1, W, 4)
            first_row = k * (rows if padded else rows_real)
            img = np.zeros((rows, W, 4), np.float32); img[:rows_real] = flat[first_row:first_row + rows_real]
            imgs.append(img)
        return imgs, np.array([st.rays_primary, st.rays_secondary, st.rays_shadow], np.int64)

    try:
        for K, band, shard, n in ((3, 8, 0, 1), (8, 8, 0, 1), (2, 8, 1, 3), (8, 8, 0, 8), (5, 16, 1, 2), (1, 8, 0, 1)):
            frames = [frame_inputs(k) for k in range(K)]
            a_imgs, a_rays = one_by_one(frames, band, shard, n)
            b_imgs, b_rays = batched(frames, band, shard, n, update=False)
            rows_real = ctx.shard_rows(H, band, shard, n)
            for k in range(K):
                assert np.array_equal(a_imgs[k][:rows_real], b_imgs[k][:rows_real]), (K, band, shard, n, k)
            assert np.array_equal(a_rays, b_rays), (K, a_rays, b_rays)
            assert a_rays[1] > 0 and a_rays[2] > 0
            # a second batch on the same context as a refit (update = 1) of the first
            frames2 = [frame_inputs(k + 3) for k in range(K)]
            a2, r2 = one_by_one(frames2, band, shard, n)
            b2, q2 = batched(frames, band, shard, n, update=False)
            b2, q2 = batched(frames2, band, shard, n, update=True)
            for k in range(K):
                assert np.array_equal(a2[k][:rows_real], b2[k][:rows_real]), ("refit", K, k)
            assert np.array_equal(r2, q2)
        # a frame of the batch against the oracle
        frames = [frame_inputs(k) for k in range(4)]
        b_imgs, _ = batched(frames, 8, 0, 1, update=False)
        sp.set_instances(frames[2][0]); sp.set_uniforms(frames[2][1])
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(b_imgs[2][:H], sp.orc, W, H, ref=ref)
        ctx.set_batch(np.stack([f[0] for f in frames]), np.concatenate([f[1] for f in frames]))
        with pytest.raises(RtError):
            ctx.trace(W, H)                      # a context that holds a batch renders it with rt_trace_shard_batch
        # a k_tail fault in a pass (forced on the host side): the WHOLE pass is rendered again from the state it was submitted with
        c2 = RtContext(0)
        try:
            scenes.ScenePair(sp.geom_paths, sp.instances, sp.uniforms, sky=sp.sky, ctx=c2)
            c2.set_param("tail_kernel", 2)
            c2.set_batch(np.stack([f[0] for f in frames]), np.concatenate([f[1] for f in frames]))
            buf = torch.zeros((4, H, W, 4), dtype=torch.float32, device="cuda:0")
            c2.set_param("debug_force_tail_fault", 1)
            c2.trace_shard_batch(W, H, 8, 0, 1, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
            st = c2.stats()
            assert st.tail_faults == 1 and st.frames_rerendered == 1
            got = buf.cpu().numpy()
            for k in range(4):
                assert np.array_equal(got[k], b_imgs[k][:H]), k
        finally:
            c2.close()
    finally:
        ctx.set_instances(sp.instances)
    # 17 instances per frame (more instance records than the kernels stage in LDS), glass centre: bounces through k_tail
    wl = workloads.make("cfg5", RES)
    wl.apply(ctx, sky=scenes.synthetic_skybox(64))
    W, H = 240, 136
    inst0 = np.ascontiguousarray(wl.instances, INSTANCE_DTYPE)
    frames = []
    for k in range(4):
        inst = inst0.copy()
        inst["transform"][:, 3] += 0.15 * k          # the whole ring drifts along x
        u = wl.uniforms.copy(); u[0]["center_object_type"] = 2
        u[0]["position"][:3] = (0.3 * k, 3.0, 24.0)
        frames.append((inst, u))
    a_imgs, a_rays = one_by_one(frames, 8, 0, 1)
    b_imgs, b_rays = batched(frames, 8, 0, 1, update=False)
    for k in range(4):
        assert np.array_equal(a_imgs[k], b_imgs[k]), k
    assert np.array_equal(a_rays, b_rays)
    ctx.set_instances(inst0)


def test_tile_blobs_are_result_identical(ctx_alt):
    """VERDICT r3 item 1 / north_star "BVH nodes and triangle packets staged through LDS": for every 8x8-pixel tile whose entry record
    names an instance k_blob writes the nodes and triangle packets the tile's beam can touch as one blob, and k_tile generates the
    tile's primary rays and walks them through it in LDS (rt_set_param "tile_blobs"; off by default: it measured slower); rays that may still hit another instance of their
    record are handed on to the global walk with their incumbent hit.  A blob must contain everything a ray of its tile can hit:
    frames and ray counts are identical with it on and off, the frame equals the oracle's, and the statistics show the path was taken.
    Cameras: the start-up one, inside an instance's box, sheared, partly off screen and very close (blobs that do not fit), far away
    (the whole scene in a few tiles: refused blobs), behind the camera; band shards; overlapping instances (rays handed on: the
    mirror teapot behind and beside the orbiting mesh); 17 instances; a one-instance scene; odd sample counts.  Tile blobs are in the
    alt library only."""
    import torch
    ctx = ctx_alt
    arm, _ = host.armadillo_path(RES)
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 1, 0, 2, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.45)
    W, H = 408, 232

    def both(w=W, h=H):
        out = {}
        for on in (1, 0):
            ctx.set_param("tile_blobs", on)
            img, st = ctx.trace(w, h, counting=True)
            out[on] = (img, (st.rays_primary, st.rays_secondary, st.rays_shadow), st.closest_rays, st)
        ctx.set_param("tile_blobs", 0)
        assert np.array_equal(out[1][0], out[0][0]) and out[1][1] == out[0][1] and out[1][2] == out[0][2]
        assert out[0][3].tile_rays == 0 and out[0][3].blob_tiles == 0
        return out

    base_u = sp.uniforms.copy()
    try:
        out = both()
        st = out[1][3]
        assert st.blob_tiles > 100 and st.tile_rays > 0.3 * st.closest_rays, (st.blob_tiles, st.tile_rays, st.closest_rays)
        assert st.blob_nodes > st.blob_tiles and st.blob_tris > st.blob_tiles
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(out[1][0], sp.orc, W, H, ref=ref)
        assert out[1][1] == (int(rc[0]), int(rc[1]), int(rc[2]))
        for band, n in ((8, 3), (16, 2)):
            rows_max = tiling.max_shard_rows(H, band, n)
            shards = []
            for s in range(n):
                buf = torch.zeros((rows_max, W, 4), dtype=torch.float32, device="cuda:0")
                ctx.trace_shard(W, H, band, s, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
                ctx.synchronize()
                shards.append(buf.cpu().numpy())
            assert np.array_equal(tiling.assemble(shards, H, W, band), out[1][0])
        handed_on = 0
        for pos, extra in (((0.3, 0.2, 5.2), {}), ((3.5, 0.5, 9.0), {}), ((0.0, 0.0, 2000.0), {}), ((6.0, 1.0, 14.0), {}), ((-4.0, 3.0, 12.0), {"center_object_type": 2, "max_bounce_count": 5}),
                           ((0.0, 0.0, 20.0), {"forward": (0.0, 0.0, 1.0)}), ((0.0, 0.0, 20.0), {"samples_per_pixel": 3}), ((1.0, 0.4, 16.0), {"samples_per_pixel": 7})):
            u = base_u.copy()
            u[0]["position"][:3] = pos
            for k, v in extra.items():
                if k == "forward":
                    u[0][k][:3] = v
                else:
                    u[0][k] = v
            sp.set_uniforms(u)
            o = both()
            handed_on += o[1][3].tile_rays_handed_on
        u = base_u.copy()
        u[0]["right"][:3] = (1.3, 0.2, 0.1); u[0]["up"][:3] = (0.15, 0.8, -0.1); u[0]["forward"][:3] = (0.1, -0.05, -1.4)
        sp.set_uniforms(u); o2 = both()
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(o2[1][0], sp.orc, W, H, ref=ref)
        handed_on += o2[1][3].tile_rays_handed_on + st.tile_rays_handed_on
    finally:
        ctx.set_param("tile_blobs", 0)
        sp.set_uniforms(base_u)
    # the start-up pose (src/main.cpp:1805-1808): the orbiting mesh stands in FRONT of the teapot, whose box most tiles' records list as
    # a rest word — rays past the silhouette of the mesh in front have to go on to it
    scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 1, 0, 2, 2, sky=scenes.synthetic_skybox(64), ctx=ctx)
    o0 = both()
    assert handed_on + o0[1][3].tile_rays_handed_on > 0
    wl = workloads.make("cfg5", RES)
    wl.apply(ctx, sky=scenes.synthetic_skybox(64))
    o5 = both(480, 270)
    assert o5[1][3].blob_tiles > 0
    wl1 = workloads.make("cfg1", RES)
    wl1.apply(ctx)
    o1 = both(256, 256)
    assert o1[1][3].blob_tiles > 0 and o1[1][3].tile_rays_handed_on == 0


def _pixel_beam_sweep(ctx, arms):
    """Every frame of the pixel-beam tests rendered in each of `arms` — 0: one walk per ray, 1: beams for the primary rays and for the
    shadow rays of the primary hits, 2: beams for the primary rays only — with identical frames, ray counts and rays entering traversal.
    The first arm (the one with the most beams) is also checked against the oracle and against band shards, and its node visits show
    that the beams ran.  Cameras: the start-up one, inside an instance's box, sheared, partly off screen and very close, far away, behind
    the camera, axis aligned (directions that straddle an axis plane inside a pixel); band shards; overlapping instances; 17 instances;
    a one-instance scene; sample counts 1, 3, 7 (a second, partly filled sample row group); a frame size that does not fill its last tiles."""
    import torch
    top = arms[0]
    arm, _ = host.armadillo_path(RES)
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 1, 0, 2, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.45)
    W, H = 408, 232

    def both(w=W, h=H):
        out = {}
        for on in arms:
            ctx.set_param("pixel_beams", 1 if on else 0)
            ctx.set_param("shadow_beams", 1 if on == 1 else 0)   # (arm 1 runs on the alt library only)
            img, st = ctx.trace(w, h, counting=True)
            out[on] = (img, (st.rays_primary, st.rays_secondary, st.rays_shadow), st.closest_rays, st)
        ctx.set_param("pixel_beams", 1); ctx.set_param("shadow_beams", 0)
        for k in arms:
            assert np.array_equal(out[k][0], out[0][0]) and out[k][1] == out[0][1] and out[k][2] == out[0][2], (k, out[k][1], out[0][1], out[k][2], out[0][2])
        return out

    base_u = sp.uniforms.copy()
    try:
        out = both()
        # (the beams' node visits are counted per pixel: fewer than one walk per ray, even with two samples in pixels this coarse)
        assert 0 < out[top][3].node_visits < 0.9 * out[0][3].node_visits, (out[top][3].node_visits, out[0][3].node_visits)
        if 1 in arms:
            assert 0 < out[1][3].node_visits_shadow != out[2][3].node_visits_shadow, (out[1][3].node_visits_shadow, out[2][3].node_visits_shadow)   # (the shadow beams ran)
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(out[top][0], sp.orc, W, H, ref=ref)
        assert out[top][1] == (int(rc[0]), int(rc[1]), int(rc[2]))
        for band, n in ((8, 3), (16, 2)):
            rows_max = tiling.max_shard_rows(H, band, n)
            shards = []
            for s in range(n):
                buf = torch.zeros((rows_max, W, 4), dtype=torch.float32, device="cuda:0")
                ctx.trace_shard(W, H, band, s, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
                ctx.synchronize()
                shards.append(buf.cpu().numpy())
            assert np.array_equal(tiling.assemble(shards, H, W, band), out[top][0])
        for pos, extra in (((0.3, 0.2, 5.2), {}), ((3.5, 0.5, 9.0), {}), ((0.0, 0.0, 2000.0), {}), ((6.0, 1.0, 14.0), {}), ((-4.0, 3.0, 12.0), {"center_object_type": 2, "max_bounce_count": 5}),
                           ((0.0, 0.0, 20.0), {"forward": (0.0, 0.0, 1.0)}), ((0.0, 0.0, 20.0), {}), ((0.0, 0.0, 20.0), {"samples_per_pixel": 3}), ((1.0, 0.4, 16.0), {"samples_per_pixel": 7}),
                           ((1.0, 0.4, 16.0), {"samples_per_pixel": 1})):
            u = base_u.copy()
            u[0]["position"][:3] = pos
            for k, v in extra.items():
                if k == "forward":
                    u[0][k][:3] = v
                else:
                    u[0][k] = v
            sp.set_uniforms(u)
            both()
            both(203, 117)
        u = base_u.copy()
        u[0]["right"][:3] = (1.3, 0.2, 0.1); u[0]["up"][:3] = (0.15, 0.8, -0.1); u[0]["forward"][:3] = (0.1, -0.05, -1.4)
        sp.set_uniforms(u); o2 = both()
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(o2[top][0], sp.orc, W, H, ref=ref)
    finally:
        ctx.set_param("pixel_beams", 1); ctx.set_param("shadow_beams", 0)
        sp.set_uniforms(base_u)
    scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 1, 0, 2, 2, sky=scenes.synthetic_skybox(64), ctx=ctx)
    both()
    wl = workloads.make("cfg5", RES)
    wl.apply(ctx, sky=scenes.synthetic_skybox(64))
    both(480, 270)
    wl1 = workloads.make("cfg1", RES)
    wl1.apply(ctx)
    both(256, 256)


def test_pixel_beams_are_result_identical(ctx):
    """One walk per PIXEL for the primary rays (csrc/kernels_beam.inc, rt_set_param "pixel_beams", default on): the samples of a pixel
    share the camera as origin, so one lane walks the tree once for all of them — boxes against the beam of the pixel's live rays
    (conservative), triangles against every ray with the canonical test and tie rule.  Frames, ray counts and the rays that enter
    traversal are identical with it on and off, the frame equals the oracle's, and the node visits show the path was taken
    (_pixel_beam_sweep: every frame rendered with pixel beams and without)."""
    _pixel_beam_sweep(ctx, (2, 0))


def test_coincident_surfaces_of_two_instances_on_primary_rays(ctx, tmp_path):
    """The (instance, primitive) tie rule on the primary rays (k_beam with pixel beams, k_trace without): a quad that two instances
    hold with the same vertices in the same order gives both the same t bits, and the LOWER instance must win although its triangles
    have the higher primitive indices.  The instances differ in object type (mirror, diffuse), so a wrong choice changes pixels."""
    quad = [(-3.0, -2.0, 0.0), (3.0, -2.0, 0.0), (3.0, 2.0, 0.0), (-3.0, 2.0, 0.0)]
    a, b = str(tmp_path / "a.obj"), str(tmp_path / "b.obj")
    with open(a, "w") as f:                                   # prim 0 out of view, the quad as prims 1 and 2
        for v in [(50.0, 50.0, -50.0), (51.0, 50.0, -50.0), (50.0, 51.0, -50.0)] + quad:
            f.write("v %g %g %g\nvn 0 0 1\n" % v)
        f.write("f 1//1 2//2 3//3\nf 4//4 5//5 6//6\nf 4//4 6//6 7//7\n")
    with open(b, "w") as f:                                   # the same quad as prims 0 and 1
        for v in quad:
            f.write("v %g %g %g\nvn 0 0 1\n" % v)
        f.write("f 1//1 2//2 3//3\nf 1//1 3//3 4//4\n")
    ident = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    inst = [host.make_instance(ident, 0, 0), host.make_instance(ident, 1, 1)]
    geom = host.SceneGeometry([a, b])
    u = host.default_uniforms(max_bounce_count=2, samples_per_pixel=2, center_object_type=1, orbiting_object_type=0,
                              orbiting_object_primitive_offset=geom.orbiting_primitive_offset,
                              orbiting_object_vertex_offset=geom.orbiting_vertex_offset)
    sp = scenes.ScenePair([a, b], np.asarray(inst, scenes.INSTANCE_DTYPE), u,
                          sky=scenes.synthetic_skybox(64), ctx=ctx)
    rays = np.array([[x, y, 20.0, 0.001, 0.0, 0.0, -1.0, 10000.0] for x in (-2.5, 0.1, 2.0) for y in (-1.5, 0.3)], np.float32)
    o = sp.orc.intersect(rays, use_bvh=False)
    assert (o["inst"] == 0).all() and set(o["prim"]) <= {1, 2} and (o["t"] == 20.0).all()
    W, H = 200, 120
    ref, rc = sp.orc.render(W, H)
    try:
        for beams in (1, 0):
            ctx.set_param("pixel_beams", beams)
            gpu, st = ctx.trace(W, H)
            assert_frame_equals_oracle(gpu, sp.orc, W, H, ref=ref)
            assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2]))
    finally:
        ctx.set_param("pixel_beams", 1)


def test_shadow_beams_are_result_identical(ctx_alt):
    """The same for the SHADOW rays of the primary hits (k_beam_shadow, "shadow_beams", default off — it measured slower; alt library
    only): a beam seen from the light, the rays' end points measured against a common one, a pixel's rays walked in groups of like
    direction; every frame of _pixel_beam_sweep is rendered three ways (both beams, neither, primary only)."""
    _pixel_beam_sweep(ctx_alt, (1, 0, 2))


def test_pixel_beams_and_settled_shadow_rays_on_random_scenes(ctx):
    """The two paths the headline rests on, on 24 seeded random scenes: random cameras (position on a shell around the scene, looking at
    a random point of it, random roll and non-orthonormal basis in a third of the cases), 2-5 instances of teapot / cube with random
    rotation, non-uniform scale (0.3 .. 2.5), shear or mirroring and position, random object types (diffuse / mirror / glass), random
    light position, 1..8 samples, frame sizes that do not fill their tiles.  For every scene: frames and ray counts per class with
    pixel beams and shadow settlement on == both off == the oracle's (every third scene; the others compare the two GPU paths only)."""
    rng = np.random.default_rng(20260405)
    paths = [os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj")]
    geom = host.SceneGeometry(paths)

    def rot(axis, ang):
        a = np.asarray(axis, np.float64); a /= np.linalg.norm(a)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * (K @ K)

    seen = {"shadow": 0, "secondary": 0, "settled": 0, "hit": 0}
    try:
        for case in range(24):
            n_inst = int(rng.integers(2, 6))
            inst = np.zeros(n_inst, scenes.INSTANCE_DTYPE)
            for k in range(n_inst):
                M = rot(rng.normal(size=3), rng.uniform(-3.0, 3.0)) @ np.diag(rng.uniform(0.3, 2.5, size=3))
                kind = rng.integers(0, 4)
                if kind == 1:
                    M = M @ np.array([[1.0, rng.uniform(-0.6, 0.6), 0.0], [0.0, 1.0, 0.0], [rng.uniform(-0.4, 0.4), 0.0, 1.0]])   # shear
                elif kind == 2:
                    M = M @ np.diag([-1.0, 1.0, 1.0])                                                                               # mirrored
                t = rng.uniform(-5.0, 5.0, size=3)
                inst[k] = host.make_instance(np.concatenate([M, t[:, None]], axis=1).astype(np.float32).reshape(12), int(k != 0), int(rng.integers(0, 2)))
            u = host.default_uniforms(max_bounce_count=int(rng.integers(0, 4)), samples_per_pixel=int(rng.choice([1, 2, 3, 4, 4, 4, 5, 8])),
                                      center_object_type=int(rng.integers(0, 3)), orbiting_object_type=int(rng.choice([0, 0, 1, 2])),
                                      orbiting_object_primitive_offset=geom.orbiting_primitive_offset, orbiting_object_vertex_offset=geom.orbiting_vertex_offset)
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            pos = d * rng.uniform(6.0, 30.0)
            target = rng.uniform(-3.0, 3.0, size=3)
            fwd = target - pos; fwd /= np.linalg.norm(fwd)
            up0 = rng.normal(size=3); right = np.cross(fwd, up0); right /= np.linalg.norm(right); up = np.cross(right, fwd)
            if case % 3 == 2:          # a basis that is neither orthogonal nor normalised (the reference's camera can be set to anything)
                right = right * rng.uniform(0.7, 1.4) + 0.15 * up; up = up * rng.uniform(0.7, 1.3) - 0.1 * fwd
            u[0]["position"][:3] = pos; u[0]["forward"][:3] = fwd; u[0]["right"][:3] = right; u[0]["up"][:3] = up
            u[0]["light_position"][:3] = rng.uniform(-15.0, 15.0, size=3)
            sp = scenes.ScenePair(paths, inst, u, sky=scenes.synthetic_skybox(64), ctx=ctx)
            W, H = int(rng.choice([160, 203, 256])), int(rng.choice([96, 117, 144]))
            out = {}
            for on in (1, 0):
                ctx.set_param("pixel_beams", on); ctx.set_param("dead_shadow_rays", on)
                img, st = ctx.trace(W, H)
                out[on] = (img, (st.rays_primary, st.rays_secondary, st.rays_shadow), st.rays_shadow_untraced)
            assert np.array_equal(out[1][0], out[0][0]) and out[1][1] == out[0][1], (case, out[1][1], out[0][1])
            seen["shadow"] += out[1][1][2]; seen["secondary"] += int(out[1][1][1] > 0); seen["settled"] += out[1][2]; seen["hit"] += int(out[1][1][2] > 0)
            if case % 3 == 0:
                ref, rc = sp.orc.render(W, H)
                assert_frame_equals_oracle(out[1][0], sp.orc, W, H, ref=ref)
                assert out[1][1] == (int(rc[0]), int(rc[1]), int(rc[2])), case
        # (the scenes are not empty: most cameras see something diffuse, some see mirrors or glass, shadow rays are settled and walked)
        assert seen["hit"] >= 10 and seen["secondary"] >= 4 and 0 < seen["settled"] < seen["shadow"], seen
    finally:
        ctx.set_param("pixel_beams", 1); ctx.set_param("dead_shadow_rays", 1)


def _settled_shadow_frames(ctx, tag, W, H):
    """A frame with "dead_shadow_rays" on and off: identical frames and ray counts, some (not all) shadow rays settled, fewer walked."""
    out = {}
    ctx.trace(W, H)      # (so that both frames below find the light-side entry records of this scene kept)
    for on in (1, 0):
        ctx.set_param("dead_shadow_rays", on)
        img, st = ctx.trace(W, H, counting=True)
        out[on] = (img, (st.rays_primary, st.rays_secondary, st.rays_shadow), st.rays_shadow_untraced, st.node_visits_shadow)
    ctx.set_param("dead_shadow_rays", 1)
    assert np.array_equal(out[1][0], out[0][0]) and out[1][1] == out[0][1], (tag, out[1][1], out[0][1])
    assert out[0][2] == 0 and 0 < out[1][2] < out[1][1][2], (tag, out[1][2], out[1][1])
    assert out[1][3] < out[0][3], (tag, out[1][3], out[0][3])       # fewer shadow rays walked
    return out


def test_shadow_rays_that_cannot_change_their_sample_are_settled_in_k_shade(ctx):
    """src/shader.rgen:107-128 traces a shadow ray for every diffuse hit and adds `pow(0.9, i) * (diffuse + specular)` if the light is
    visible.  Where the surface AND the half vector face away from the light both terms are exactly 0: tmpColor stays Iamb*ka whether the
    ray reaches the light or not, bit for bit — k_shade writes the sample and does not queue the ray (rt_set_param "dead_shadow_rays",
    default on; rt_stats.rays_shadow still counts it, rays_shadow_untraced says how many).  Frames and ray counts are identical with the
    parameter on and off and equal the oracle's, with and without a material table (Iamb*ka of the hit's material), with the shadow
    rays in beams (alt library: test_settled_shadow_rays_with_shadow_beams), and in the bounce loop (mirror teapot: k_tail)."""
    arm, _ = host.armadillo_path(RES)
    W, H = 408, 232

    def both(tag):
        return _settled_shadow_frames(ctx, tag, W, H)

    try:
        sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 1, 0, 2, 3, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.45)
        o = both("diffuse mesh behind a mirror teapot")
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(o[1][0], sp.orc, W, H, ref=ref)
        assert o[1][1] == (int(rc[0]), int(rc[1]), int(rc[2]))
        # the light on the far side: most visible surfaces face away from it
        u = sp.uniforms.copy(); u[0]["light_position"][:3] = (-6.0, -3.0, -20.0)
        sp.set_uniforms(u)
        o2 = both("light behind the scene")
        assert o2[1][2] > 0.3 * o2[1][1][2], (o2[1][2], o2[1][1])
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(o2[1][0], sp.orc, W, H, ref=ref)
        assert o2[1][1] == (int(rc[0]), int(rc[1]), int(rc[2]))
        # a material table: the settled colour is Iamb*ka of the hit's material
        inst = [host.make_instance(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), 0, 0)]
        um = host.default_uniforms(max_bounce_count=2, samples_per_pixel=2, center_object_type=0, orbiting_object_type=0)
        spm = scenes.ScenePair([os.path.join(RES, "cube_scene.obj")], inst, um, sky=scenes.synthetic_skybox(64), ctx=ctx)
        spm.set_materials(spm.geom.materials, spm.geom.prim_material)
        W, H = 256, 256
        om = both("materials")
        ref, rc = spm.orc.render(W, H)
        assert_frame_equals_oracle(om[1][0], spm.orc, W, H, ref=ref)
        assert om[1][1] == (int(rc[0]), int(rc[1]), int(rc[2]))
    finally:
        ctx.set_param("dead_shadow_rays", 1)
        ctx.set_materials(None)


def test_settled_shadow_rays_with_shadow_beams(ctx_alt):
    """The frame of test_shadow_rays_that_cannot_change_their_sample_are_settled_in_k_shade with the shadow rays of the primary hits in
    beams (k_beam_shadow, "shadow_beams", alt library only): settling still gives the same frame, and fewer rays are walked."""
    ctx = ctx_alt
    arm, _ = host.armadillo_path(RES)
    try:
        scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 1, 0, 2, 3, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.45)
        ctx.set_param("shadow_beams", 1)
        _settled_shadow_frames(ctx, "shadow beams", 408, 232)
    finally:
        ctx.set_param("dead_shadow_rays", 1); ctx.set_param("shadow_beams", 0)


def test_jitter_table_is_bit_identical_to_evaluating_the_hash(ctx):
    """k_raygen reads (ux, uy) of every sample from a table computed once per (width, height, spp, shard layout)
    by the same device function (kernels.hip sample_uv / k_jitter_table) instead of evaluating two binary64 sines per sample and
    frame (rt_set_param "jitter_table", default on).  Frames and ray counts are identical with it on and off: whole frames, odd
    sizes that do not fill their last tiles, sample counts that need several workgroups per tile, band shards (their rows map to
    other frame rows), more frame sizes than the scene keeps tables for (the oldest is dropped), and frame slots sharing a table."""
    import torch
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 1, 0, 2, 4, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.2)
    base_u = sp.uniforms.copy()

    def both(w, h, spp):
        u = base_u.copy(); u[0]["samples_per_pixel"] = spp
        sp.set_uniforms(u)
        out = {}
        for on in (1, 0, 1):
            ctx.set_param("jitter_table", on)
            img, st = ctx.trace(w, h)
            if on in out:
                assert np.array_equal(out[on][0], img)       # the second frame finds the table
            out[on] = (img, (st.rays_primary, st.rays_secondary, st.rays_shadow))
        assert np.array_equal(out[1][0], out[0][0]) and out[1][1] == out[0][1], (w, h, spp)
        return out[1][0]

    try:
        full = both(200, 120, 4)
        ref, _ = sp.orc.render(200, 120)
        assert_frame_equals_oracle(full, sp.orc, 200, 120, ref=ref)
        for w, h, spp in ((203, 117, 4), (64, 64, 1), (131, 77, 3), (96, 40, 7), (40, 24, 9), (8, 8, 2), (1, 1, 4), (333, 5, 2), (17, 190, 5), (72, 72, 4)):
            both(w, h, spp)                                   # > 8 sizes: tables are dropped and rebuilt
        both(200, 120, 4)
        u = base_u.copy(); u[0]["samples_per_pixel"] = 4
        sp.set_uniforms(u)
        W, H = 200, 120
        for on in (1, 0):
            ctx.set_param("jitter_table", on)
            for band, n in ((8, 3), (5, 2)):
                rows_max = tiling.max_shard_rows(H, band, n)
                shards = []
                for s in range(n):
                    buf = torch.zeros((rows_max, W, 4), dtype=torch.float32, device="cuda:0")
                    ctx.trace_shard(W, H, band, s, n, buf.data_ptr(), buf.numel() * 4, torch.cuda.current_stream().cuda_stream)
                    ctx.synchronize()
                    shards.append(buf.cpu().numpy())
                assert np.array_equal(tiling.assemble(shards, H, W, band), full), (on, band, n)
        ctx.set_param("jitter_table", 1)
        slots = [ctx.frame_slot() for _ in range(2)]
        try:
            for c in slots:
                c.set_instances(sp.instances); c.set_uniforms(u)
                c.trace_async(W, H)
            for c in slots:
                img, _ = c.trace_wait()
                assert np.array_equal(img, full)
        finally:
            for c in slots:
                c.close()
    finally:
        ctx.set_param("jitter_table", 1)
        sp.set_uniforms(base_u)


def test_entry_records_keep_the_far_flag_of_the_instance_they_enter(ctx):
    """a primary ray that starts from an entry record which names an instance is moved into that instance's
    object space at refill; whether it is FAR there (kernels.hip quant_far) must be decided against the MESH's quantisation, not
    against the TLAS's.  A small mesh (the cube: 3e-5 units per quantum) inside a large TLAS (a second instance 3000 units away
    makes the TLAS quantum 0.05), seen through a long lens from 50 to 20 000 mesh extents away — far in object space, not far in
    world space: frames and ray counts with entry records equal the frames without them and the oracle's."""
    cube = os.path.join(RES, "cube.obj")
    eye = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    for scale in (1.0, 0.01):       # (an instance scale of 0.01 multiplies every object-space distance by 100)
        small = eye.copy(); small[0] = small[5] = small[10] = scale
        small[3], small[7], small[11] = 0.3, -0.2, 0.1
        away = eye.copy(); away[3], away[7], away[11] = 3000.0, 40.0, -2500.0
        inst = [host.make_instance(small, 0, 0), host.make_instance(away, 1, 1)]
        u = host.default_uniforms(max_bounce_count=1, samples_per_pixel=2, center_object_type=0, orbiting_object_type=1)
        sp = scenes.ScenePair([cube, cube], inst, u, sky=scenes.synthetic_skybox(64), ctx=ctx)
        base_u = sp.uniforms.copy()
        try:
            for dist, off in ((100.0, (0.0, 0.0, 1.0)), (400.0, (0.6, 0.3, 0.74)), (2500.0, (1.0, 0.002, 0.001)), (9000.0, (0.001, 1.0, 0.003)), (40000.0 if scale < 1.0 else 7000.0, (0.7, 0.0, 0.7))):
                dirn = np.asarray(off, np.float64); dirn /= np.linalg.norm(dirn)
                pos = np.array([0.3, -0.2, 0.1]) + dirn * dist * scale
                fwd = -dirn
                right = np.cross(fwd, [0.0, 1.0, 0.0] if abs(fwd[1]) < 0.9 else [1.0, 0.0, 0.0]); right /= np.linalg.norm(right)
                up = np.cross(right, fwd)
                uu = base_u.copy()
                uu[0]["position"][:3] = pos
                uu[0]["right"][:3] = right; uu[0]["up"][:3] = up
                uu[0]["forward"][:3] = fwd * (dist / 4.0)       # long lens: the cube fills a good part of the frame
                sp.set_uniforms(uu)
                out = {}
                for on in (1, 0):
                    ctx.set_param("entry_points", on)
                    img, st = ctx.trace(136, 104)
                    out[on] = (img, (st.rays_primary, st.rays_secondary, st.rays_shadow))
                ctx.set_param("entry_points", 1)
                assert np.array_equal(out[1][0], out[0][0]) and out[1][1] == out[0][1], (scale, dist)
                ref, rc = sp.orc.render(136, 104)
                assert_frame_equals_oracle(out[1][0], sp.orc, 136, 104, ref=ref)
                assert out[1][1] == (int(rc[0]), int(rc[1]), int(rc[2])) and out[1][1][2] > 500, (scale, dist, out[1][1])
        finally:
            ctx.set_param("entry_points", 1)


def test_kept_shadow_entry_records_follow_the_light_and_the_instances(ctx):
    """rt_set_param "shadow_entry" 2 (the default): the records of the cube around the light depend on the light, the instances and the
    trees only, so they are KEPT while those stand still — built in a context's first frame and in the second consecutive frame with a new
    key, used from then on (whatever the camera does), dropped the moment the light moves or rt_set_instances runs (an animated loop builds
    them once, at its first frame, and never again).  Every frame of a sequence that mixes all of that equals the frame rendered without
    records, and the shadow rays' node visits tell which frames used them."""
    arm, _ = host.armadillo_path(RES)
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 0, 0, 2, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.45)
    W, H = 320, 200
    base_u = sp.uniforms.copy()
    anim = host.SceneAnimation(); anim.animate(0.45)

    def frame():
        img, st = ctx.trace(W, H, counting=True)
        return img, st.node_visits_shadow / max(1, st.rays_shadow)

    def reference():   # the same frame without records (changing the parameter drops what is kept)
        ctx.set_param("shadow_entry", 0)
        out = frame()
        ctx.set_param("shadow_entry", 2)
        return out

    try:
        ref, v_root = reference()
        seq = []
        for _ in range(3):      # first frame after the reset: built at once (optimistic start); then kept
            img, v = frame(); seq.append(v); assert np.array_equal(img, ref)
        assert seq[0] < 0.85 * v_root and seq[1] == seq[0] and seq[2] == seq[0], (v_root, seq)
        # the camera moves: the records do not depend on it — no rebuild, still used
        u = base_u.copy(); u[0]["position"][:3] = np.asarray(u[0]["position"][:3]) + np.float32([0.4, 0.2, -0.3])
        sp.set_uniforms(u)
        img, v = frame()
        ref_cam, v_cam_root = reference()
        assert np.array_equal(img, ref_cam) and v < 0.85 * v_cam_root
        frame()                                                                 # (records exist again after the reference's reset)
        # the light moves: dropped at once (this frame walks from the TLAS root), rebuilt one frame later, kept after that
        u2 = u.copy(); u2[0]["light_position"][:3] = (1.5, 3.0, 4.0)
        sp.set_uniforms(u2)
        img_a, va = frame()
        img_b, vb = frame()
        img_c, vc = frame()
        ref_l, v_l_root = reference()
        assert np.array_equal(img_a, ref_l) and np.array_equal(img_b, ref_l) and np.array_equal(img_c, ref_l)
        assert va == v_l_root and vb < 0.85 * v_l_root and vc == vb, (v_l_root, va, vb, vc)
        frame()
        # the instances move every frame (the reference's loop): dropped, never rebuilt, every frame exact
        for k in range(3):
            anim.animate(0.45 + 0.01 * (k + 1))
            ctx.set_instances(anim.instances((0, 1)), update=True)
            img2, vk = frame()
            anim_ref = RtContext(0)
            try:
                sp2 = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 0, 0, 2, 2, sky=scenes.synthetic_skybox(64), ctx=anim_ref, time_param=0.45)
                anim_ref.set_param("shadow_entry", 0)
                anim_ref.set_instances(anim.instances((0, 1)))
                anim_ref.set_uniforms(u2)
                img0, st0 = anim_ref.trace(W, H, counting=True)
            finally:
                anim_ref.close()
            assert np.array_equal(img2, img0)
            assert vk == st0.node_visits_shadow / max(1, st0.rays_shadow), (k, vk)
    finally:
        ctx.set_param("shadow_entry", 2)
        sp.set_uniforms(base_u)


def test_shadow_entry_points_are_result_identical(ctx):
    """Shadow rays all end (within 0.01) at the light, so k_entry also gives every tile of a cube around the light an entry list
    and k_shade tells each shadow ray its tile (rt_set_param "shadow_entry", default on; "light_tiles" per cube side).  Any-hit
    queries only ask WHETHER something is hit, so the lists must contain every possible occluder: frames and ray counts are
    identical with the lists on and off, for lights outside, between and INSIDE the meshes' boxes, far away, on a cube-face
    diagonal, next to a surface, for several light_tiles, for diffuse-on-diffuse scenes (every primary hit casts a shadow
    ray), with 17 instances, and the frame equals the oracle's; shadow node visits per ray drop."""
    arm, _ = host.armadillo_path(RES)
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 0, 0, 2, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.45)
    W, H = 408, 232

    def both(w=W, h=H):
        out = {}
        for on in (1, 0):
            ctx.set_param("shadow_entry", on)
            img, st = ctx.trace(w, h, counting=True)
            out[on] = (img, (st.rays_primary, st.rays_secondary, st.rays_shadow), st.node_visits_shadow)
        ctx.set_param("shadow_entry", 0)
        assert out[1][1] == out[0][1]
        assert np.array_equal(out[1][0], out[0][0]), "shadow entry lists changed %d pixels" % int((out[1][0] != out[0][0]).any(axis=2).sum())
        return out

    base_u = sp.uniforms.copy()
    try:
        out = both()
        assert out[1][1][2] > 5000
        assert out[1][2] < 0.8 * out[0][2], (out[1][2], out[0][2])
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(out[1][0], sp.orc, W, H, ref=ref)
        assert out[1][1] == (int(rc[0]), int(rc[1]), int(rc[2]))
        for light in ((0.0, 0.0, 12.0), (0.3, 0.2, 5.2), (0.0, 3.0, 2.5), (1000.0, 800.0, 600.0), (4.0, 4.0, 4.0), (-6.0, 0.01, 0.0), (0.0, 0.0, 0.0), (2.9, 0.0, 5.0)):
            u = base_u.copy()
            u[0]["light_position"][:3] = light
            sp.set_uniforms(u); both()
        sp.set_uniforms(base_u)
        for lt in (8, 37, 512):
            ctx.set_param("light_tiles", lt)
            o = both()
            assert np.array_equal(o[1][0], out[1][0])
        ctx.set_param("light_tiles", 256)
    finally:
        ctx.set_param("shadow_entry", 2); ctx.set_param("light_tiles", 256)
        sp.set_uniforms(base_u)
    wl = workloads.make("cfg5", RES)
    wl.apply(ctx, sky=scenes.synthetic_skybox(64))
    ctx.set_param("entry_max_instances", 64)
    try:
        o5 = both(480, 270)
    finally:
        ctx.set_param("entry_max_instances", 32)
    assert o5[1][2] < o5[0][2]
    wl1 = workloads.make("cfg1", RES)
    wl1.apply(ctx)
    both(256, 256)


def test_tail_fault_rerenders_the_submitted_frame_on_the_shard_and_multi_gpu_paths(ctx):
    """the k_tail fault fallback on the rt_trace_shard path.  (1) The re-render uses the uniforms and instance
    records the frame was SUBMITTED with, even if rt_set_uniforms / one rt_set_instances ran before the frame was collected;
    two instance updates before collecting make the frame unrecoverable and that is reported, not papered over.  (2) A fault in
    an earlier frame of a stream of uncollected frames is still counted (sticky device-side total) and switches the slot off
    k_tail.  (3) librt_multi.so (loopback, 3 logical devices): rtm_trace_wait learns of the re-render (frames_rerendered) and
    gathers, de-interleaves and copies the slot again, so the frame it hands out is complete."""
    import torch
    from vulkan_raytracing_amd import multi
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 2, 1, 12, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.5)
    W, H = 160, 96
    good, st0 = ctx.trace(W, H)
    u_other = sp.uniforms.copy()
    u_other[0]["position"][:3] = (3.0, 2.0, 14.0)
    inst_other = sp.instances.copy()
    inst_other[1]["transform"][3] += 1.5
    stream = torch.cuda.Stream()
    buf = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    c2 = RtContext(0)
    try:
        scenes.ScenePair(sp.geom_paths, sp.instances, sp.uniforms, sky=sp.sky, ctx=c2)
        c2.set_param("tail_kernel", 2)
        # (1) uniforms and ONE instance update between submit and collect
        c2.set_param("debug_force_tail_fault", 1)
        c2.trace_shard(W, H, H, 0, 1, buf.data_ptr(), buf.numel() * 4, stream.cuda_stream)
        c2.set_uniforms(u_other)
        c2.set_instances(inst_other, update=True)
        st = c2.stats()
        assert st.tail_faults == 1 and st.frames_rerendered == 1
        assert np.array_equal(buf.cpu().numpy(), good), "the re-rendered frame is not the submitted one"
        c2.trace_shard(W, H, H, 0, 1, buf.data_ptr(), buf.numel() * 4, stream.cuda_stream)     # the new state renders a different frame, no re-render
        st = c2.stats()
        assert st.frames_rerendered == 0 and not np.array_equal(buf.cpu().numpy(), good)
        # two updates before collecting: the frame's records are gone, and the call says so
        c2.set_uniforms(sp.uniforms); c2.set_instances(sp.instances, update=True)
        c2.set_param("debug_force_tail_fault", 2)      # 2: also re-arms k_tail on this context
        c2.trace_shard(W, H, H, 0, 1, buf.data_ptr(), buf.numel() * 4, stream.cuda_stream)
        c2.set_instances(inst_other, update=True); c2.set_instances(sp.instances, update=True)
        with pytest.raises(RtError) as e:
            c2.stats()
        assert "cannot be rendered again" in str(e.value)
        c2.trace_shard(W, H, H, 0, 1, buf.data_ptr(), buf.numel() * 4, stream.cuda_stream)
        c2.synchronize()
        assert np.array_equal(buf.cpu().numpy(), good)
    finally:
        c2.close()
    # (3) three logical devices, two slots: a forced fault on every slot of every device
    m = multi.RtMulti([0, 0, 0], 2, loopback=True)
    try:
        g = sp.geom
        m.upload_geometry(g.verts, g.idx, g.ranges)
        m.set_instances(sp.instances); m.set_uniforms(sp.uniforms); m.set_skybox(sp.sky)
        m.set_param("tail_kernel", 2)
        m.trace_async(0, W, H)
        ok, s_ok = m.trace_wait(0)
        assert np.array_equal(ok, good) and s_ok.frames_rerendered == 0
        m.set_param("debug_force_tail_fault", 1)
        m.trace_async(1, W, H); m.trace_async(0, W, H)
        for slot in (1, 0):
            img, s1 = m.trace_wait(slot)
            assert s1.frames_rerendered == 3 and s1.tail_faults == 3, (s1.frames_rerendered, s1.tail_faults)
            assert np.array_equal(img, good), "slot %d: the gathered frame is stale" % slot
            assert (s1.rays_primary, s1.rays_secondary, s1.rays_shadow) == (st0.rays_primary, st0.rays_secondary, st0.rays_shadow)
    finally:
        m.close()


def test_bgra8_surface_byte_order_and_materials_on_the_multi_gpu_host(ctx, tmp_path):
    """Row n2: the reference's storage image has the surface format, normally B8G8R8A8 (src/main.cpp:1204, 1899):
    rt_set_param "output_bgra8" stores the 8-bit frame in that byte order = the RGBA8 frame with R and B swapped, on the
    single-GPU path, through rt_assemble_shards (3 logical devices) and in rt_headless --bgra8.  Row n4 on the multi-GPU
    host: rtm_set_materials / rtm_set_instance_types give the frame the single-GPU path renders with the same table."""
    import subprocess
    from vulkan_raytracing_amd import multi
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 1, 0, 2, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.3)
    W, H = 200, 120
    try:
        ctx.set_param("output_rgba8", 1)
        rgba, _ = ctx.trace(W, H)
        ctx.set_param("output_bgra8", 1)
        bgra, _ = ctx.trace(W, H)
    finally:
        ctx.set_param("output_rgba8", 0)
    assert rgba.dtype == np.uint8 and rgba.std() > 5 and np.array_equal(bgra[..., [2, 1, 0, 3]], rgba)
    g = sp.geom
    n_prims = len(g.idx) // 3
    from vulkan_raytracing_amd.api import MATERIAL_DTYPE, MATERIAL_TYPE_OF_INSTANCE
    table = np.zeros(3, MATERIAL_DTYPE)
    table[0] = ((0.1, 0.3, 0.1), 100.0, (0.2, 1.0, 0.2), 1.52, (0.8, 0.8, 0.8), MATERIAL_TYPE_OF_INSTANCE)
    table[1] = ((0.3, 0.1, 0.1), 20.0, (0.9, 0.3, 0.2), 1.33, (0.5, 0.5, 0.5), 0)
    table[2] = ((0.1, 0.1, 0.3), 60.0, (0.2, 0.3, 0.9), 1.45, (0.9, 0.9, 0.9), 2)
    pm = (np.arange(n_prims) % 3).astype(np.uint32)
    ctx.set_materials(table, pm)
    ctx.set_instance_types([2, 0])
    try:
        ref_mat, st_ref = ctx.trace(W, H)
        ctx.set_param("output_bgra8", 1)
        ref_mat8, _ = ctx.trace(W, H)
    finally:
        ctx.set_param("output_rgba8", 0)
        ctx.set_materials(None)
        ctx.set_instance_types(None)
    m = multi.RtMulti([0, 0, 0], 2, loopback=True)
    try:
        m.upload_geometry(g.verts, g.idx, g.ranges)
        m.set_instances(sp.instances); m.set_uniforms(sp.uniforms); m.set_skybox(sp.sky)
        m.set_materials(table, pm)
        m.set_instance_types([2, 0])
        m.trace_async(1, W, H)
        img, st = m.trace_wait(1)
        assert np.array_equal(img, ref_mat)
        assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (st_ref.rays_primary, st_ref.rays_secondary, st_ref.rays_shadow)
        m.set_param("output_bgra8", 1)
        m.trace_async(0, W, H)
        img8, _ = m.trace_wait(0)
        assert img8.dtype == np.uint8 and np.array_equal(img8, ref_mat8)
    finally:
        m.close()
    exe = os.path.join(scenes.ROOT, "rt_headless")
    common = ["--width", "160", "--height", "96", "--frames", "2", "--dt", "0.5", "--bounce", "2", "--spp", "2", "--frames-in-flight", "2",
              "--center", os.path.join(RES, "teapot.obj"), "--orbiting", os.path.join(RES, "cube.obj"), "--skybox", os.path.join(RES, "skybox_texture_test")]
    raw = {}
    for name, extra in (("a", ["--rgba8"]), ("b", ["--bgra8"])):
        out = str(tmp_path / name)
        r = subprocess.run([exe] + common + extra + ["--out", out], cwd=scenes.ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-500:] + r.stderr[-1000:]
        raw[name] = open(out + ".ppm", "rb").read()
    assert raw["a"] == raw["b"]                                    # the PPM view is swizzled back
    b = np.frombuffer(open(str(tmp_path / "b") + ".bgra", "rb").read(), np.uint8).reshape(96, 160, 4)
    ppm = np.frombuffer(raw["b"][raw["b"].index(b"255\n") + 4:], np.uint8).reshape(96, 160, 3)
    assert np.array_equal(b[..., [2, 1, 0]], ppm)


def test_bench_one_process_multi_gpu_host_reassembles_the_same_frame(tmp_path):
    """bench.py --host multi: ONE process drives N (here 2 logical, --loopback) devices through librt_multi.so; its frame equals
    the single-GPU bench frame bit for bit and the line carries n_gpus."""
    import json
    import subprocess
    import sys
    a, b = str(tmp_path / "one.pfm"), str(tmp_path / "multi.pfm")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(scenes.ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-extras", "--save-image", a],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(scenes.ROOT, "bench.py"), "--gpus", "2", "--host", "multi", "--loopback", "--steps", "4", "--warmup", "2",
                        "--no-extras", "--save-image", b], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
    assert line["n_gpus"] == 2 and line["config"]["host"] == "multi" and line["value"] > 0
    assert line["config"]["frames_per_pass"] == 4       # (round 4: the devices render passes of frames, one gather per pass)
    assert open(a, "rb").read() == open(b, "rb").read()
    # the animated loop: every frame of a pass has its own instances (rtm_set_batch); 3 logical devices, passes of 3 frames
    a2, b2 = str(tmp_path / "one_anim.pfm"), str(tmp_path / "multi_anim.pfm")
    r = subprocess.run([sys.executable, os.path.join(scenes.ROOT, "bench.py"), "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--no-extras", "--animate", "--save-image", a2],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([sys.executable, os.path.join(scenes.ROOT, "bench.py"), "--gpus", "3", "--host", "multi", "--loopback", "--steps", "5", "--warmup", "2", "--batch", "3",
                        "--no-extras", "--animate", "--save-image", b2], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(a2, "rb").read() == open(b2, "rb").read()
    assert open(a2, "rb").read() != open(a, "rb").read()


def test_far_origins_up_to_the_pipelines_tmax_and_beyond(ctx):
    """the conservative box test from FAR origins.  The pipeline's tmax is 10000 (src/shader.rgen:86-87) and
    the camera flies freely, so hits from thousands of units away are reachable; there the rounding of (plane - origin) exceeds
    the margin of the stored planes and used to lose a record in 40 000 from 20 000 units.  Rays whose origin is that far now
    take the generic visit with a per-axis widened slab test (kernels.hip quant_far): hit records must equal the oracle's brute
    force bit for bit from 20 to 20 000 units (twice the pipeline's tmax), closest hit and any hit, through instance transforms,
    a third of the rays nearly parallel to a coordinate axis; and a frame rendered from 5000 units away equals the oracle's."""
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj"), 1, 0, 1, 1, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.3)
    rng = np.random.default_rng(5)
    # (beyond ~4 x tmax a binary32 ray is too coarse for any claim: ulp(t) = 0.004 at 60 000 units, and 1 record in 30 000 still
    # differs there — out of the pipeline's reach, src/shader.rgen:86-87 ends every ray at 10 000)
    for dist in (20.0, 700.0, 2000.0, 5000.0, 10000.0, 14000.0, 20000.0):
        n = 30000
        o = rng.normal(size=(n, 3)); o /= np.linalg.norm(o, axis=1, keepdims=True); o *= dist
        tgt = rng.uniform(-2.5, 2.5, (n, 3)); tgt[:, 1] = rng.uniform(0, 1.6, n)
        half = rng.random(n) < 0.5
        tgt[half] = rng.uniform(-1.2, 1.2, (int(half.sum()), 3))
        # a third of the rays nearly parallel to a coordinate axis: the case no relative slack in t covers
        ax = rng.integers(0, 3, n)
        par = rng.random(n) < 0.33
        o[par] = tgt[par]
        o[par, ax[par]] += dist * rng.choice([-1.0, 1.0], int(par.sum()))
        o[par] += rng.normal(scale=1e-3, size=(int(par.sum()), 3))
        d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.zeros((n, 8), np.float32); rays[:, 0:3] = o; rays[:, 3] = 0.001; rays[:, 4:7] = d; rays[:, 7] = 1e9
        g, _ = ctx.intersect(rays)
        b = sp.orc.intersect(rays, use_bvh=False)
        same = (g["prim"] == b["prim"]) & (g["inst"] == b["inst"]) & (g["t"].view(np.uint32) == b["t"].view(np.uint32))
        assert (b["inst"] >= 0).mean() > 0.3
        assert same.all(), "from %g units: %d of %d hit records differ from brute force" % (dist, int((~same).sum()), n)
        ga, _ = ctx.intersect(rays, any_hit=True)
        assert np.array_equal(ga["inst"] >= 0, b["inst"] >= 0)
    u = sp.uniforms.copy()
    u[0]["position"][:3] = (0.0, 0.0, 5000.0)
    u[0]["forward"][:3] = (0.0, 0.0, -2000.0)       # a long lens (the shader takes the vectors as they come): the scene fills part of the frame
    sp.set_uniforms(u)
    img, st = ctx.trace(200, 120)
    ref, rc = sp.orc.render(200, 120)
    assert_frame_equals_oracle(img, sp.orc, 200, 120, ref=ref)
    assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (int(rc[0]), int(rc[1]), int(rc[2])) and st.rays_secondary > 100


def test_packet_kernel_is_result_identical(ctx_alt):
    """k_packet (rt_set_param "packet_trace": one wavefront walks a 64-ray chunk together — wave-uniform stack, scalar node and
    triangle loads, every lane tests every visited node) is an alternative traversal kernel for the primary and the shadow rays,
    off by default because it measured slower.  A lane tests candidates its own ray would never have reached, so it only works
    because results do not depend on the set or order of candidates tested: frames and ray counts equal the one-lane-per-ray
    kernels', with and without entry records, for the shadow-ray records too, and record-level rays (incoherent: the worst case
    for a packet) equal the oracle's brute force, closest hit and any hit.  (librt_mi355x_alt.so: not in the product library.)"""
    ctx = ctx_alt
    arm, _ = host.armadillo_path(RES)
    sp = scenes.two_object_scene(os.path.join(RES, "teapot.obj"), arm, 2, 0, 4, 2, sky=scenes.synthetic_skybox(64), ctx=ctx, time_param=0.45)
    W, H = 328, 203
    try:
        base, st0 = ctx.trace(W, H)
        for params in ({"packet_trace": 1}, {"packet_trace": 1, "entry_points": 0}, {"packet_trace": 1, "shadow_entry": 1}, {"packet_trace": 1, "primary_cover": 0}):
            for k, v in params.items():
                ctx.set_param(k, v)
            img, st = ctx.trace(W, H)
            assert np.array_equal(img, base), params
            assert (st.rays_primary, st.rays_secondary, st.rays_shadow) == (st0.rays_primary, st0.rays_secondary, st0.rays_shadow)
            for k in params:
                ctx.set_param(k, {"packet_trace": 0, "entry_points": 1, "shadow_entry": 0, "primary_cover": 1}[k])
        ref, rc = sp.orc.render(W, H)
        assert_frame_equals_oracle(base, sp.orc, W, H, ref=ref)
        rng = np.random.default_rng(11)
        n = 20000
        o = rng.normal(size=(n, 3)) * 6.0
        d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.zeros((n, 8), np.float32); rays[:, 0:3] = o; rays[:, 3] = 0.001; rays[:, 4:7] = d; rays[:, 7] = 1e4
        b = sp.orc.intersect(rays, use_bvh=False)
        ctx.set_param("packet_trace", 2)
        g, _ = ctx.intersect(rays)
        assert ((g["prim"] == b["prim"]) & (g["inst"] == b["inst"]) & (g["t"].view(np.uint32) == b["t"].view(np.uint32))).all()
        ga, _ = ctx.intersect(rays, any_hit=True)
        assert np.array_equal(ga["inst"] >= 0, b["inst"] >= 0)
    finally:
        for k, v in {"packet_trace": 0, "entry_points": 1, "shadow_entry": 0, "primary_cover": 1}.items():
            ctx.set_param(k, v)
