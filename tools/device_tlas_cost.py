"""What the device TLAS (rt_set_instances_device) costs against the host TLAS (rt_set_instances), written to one JSON file.

  per_call      wall time of one call + rt_synchronize, build (update 0) and refit (update 1), at 17 .. 262 144 instances: median and
                spread over --calls calls after --warmup calls (host clock around call + synchronise)
  animated      ms per step of the animated loop with 16 384 instances, 4 frame slots in flight, one update per frame, both paths
  cfg5_static   cfg5 frame time (full size) from the device LBVH TLAS against the host SAH TLAS (tree quality costs traversal time)
  kernel_stats  --kernel-stats DIR merges the TLAS kernels of a rocprofv3 --kernel-trace --stats run of `--kernels-only` (a run of
                its own: tracing slows the host)

python3 tools/device_tlas_cost.py --out device_tlas_cost_results.json
rocprofv3 --kernel-trace --stats --output-format csv -d tlas_prof -o tlas -- python3 tools/device_tlas_cost.py --kernels-only
python3 tools/device_tlas_cost.py --out device_tlas_cost_results.json --kernel-stats tlas_prof"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vulkan_raytracing_amd import RtContext, host, workloads  # noqa: E402
from vulkan_raytracing_amd.api import INSTANCE_DTYPE  # noqa: E402

RES = os.path.join(ROOT, "resources")
PATHS = [os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj")]
COUNTS = [17, 1024, 16384, 65535, 262144]


def field(n, seed=0):
    """n small teapots and cubes at seeded random positions in a cube that grows with n (about constant density)"""
    rng = np.random.default_rng(seed)
    ext = 2.0 * max(1.0, n ** (1 / 3)) * 0.5
    inst = np.zeros(n, INSTANCE_DTYPE)
    s = rng.uniform(0.05, 0.2, n).astype(np.float32)
    tr = np.zeros((n, 12), np.float32)
    tr[:, 0] = tr[:, 5] = tr[:, 10] = s
    tr[:, 3], tr[:, 7], tr[:, 11] = (rng.uniform(-ext, ext, n).astype(np.float32) for _ in range(3))
    inst["transform"] = tr
    mesh = (np.arange(n) % 2).astype(np.uint64)
    inst["mesh"] = mesh
    inst["custom_index_and_mask"] = mesh.astype(np.uint32) | np.uint32(0xFF << 24)
    return inst


def moved(inst, vel, k):
    out = inst.copy()
    tr = out["transform"]
    tr[:, 3] += np.float32(k) * vel[:, 0]; tr[:, 7] += np.float32(k) * vel[:, 1]; tr[:, 11] += np.float32(k) * vel[:, 2]
    out["transform"] = tr
    return out


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max()),
            "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90)), "calls": len(a)}


def scene(ctx, inst, max_bounce=1):
    geom = host.SceneGeometry(PATHS)
    ctx.upload_geometry(geom.verts, geom.idx, geom.ranges)
    ctx.set_instances(inst)
    ctx.set_uniforms(host.default_uniforms(max_bounce_count=max_bounce, samples_per_pixel=1, center_object_type=1, orbiting_object_type=0,
                                           orbiting_object_primitive_offset=geom.orbiting_primitive_offset,
                                           orbiting_object_vertex_offset=geom.orbiting_vertex_offset))


def per_call(args, torch):
    out = {}
    for n in COUNTS:
        ctx = RtContext(0)
        inst = field(n, seed=n)
        vel = np.random.default_rng(1).normal(scale=0.01, size=(n, 3)).astype(np.float32)
        scene(ctx, inst)
        frames = [moved(inst, vel, k) for k in range(4)]
        dev = [torch.from_numpy(f.view(np.uint8).reshape(-1, 64).copy()).to("cuda:0") for f in frames]
        torch.cuda.synchronize()
        row = {}
        for path in ("host", "device"):
            for mode, update in (("build", False), ("refit", True)):
                ms = []
                for k in range(args.warmup + args.calls):
                    t0 = time.perf_counter()
                    if path == "host":
                        ctx.set_instances(frames[k % 4], update=update)
                    else:
                        ctx.set_instances_device(dev[k % 4], update=update)
                    ctx.synchronize()
                    if k >= args.warmup:
                        ms.append(1e3 * (time.perf_counter() - t0))
                row["%s_%s" % (path, mode)] = stats(ms)
        out[str(n)] = row
        print("per call, %d instances: %s" % (n, {k: round(v["median_ms"], 3) for k, v in row.items()}), flush=True)
        ctx.close()
    return out


def animated(args, torch, n=16384, slots=4, W=640, H=360):
    inst = field(n, seed=5)
    vel = np.random.default_rng(2).normal(scale=0.01, size=(n, 3)).astype(np.float32)
    ctx = RtContext(0)
    scene(ctx, inst)
    ring = [ctx] + [ctx.frame_slot() for _ in range(slots - 1)]
    for c in ring[1:]:
        c.set_uniforms(host.default_uniforms(max_bounce_count=1, samples_per_pixel=1, center_object_type=1, orbiting_object_type=0))
    words = torch.from_numpy(inst.view(np.float32).reshape(-1, 16).copy()).to("cuda:0")
    vel_t = torch.from_numpy(vel).to("cuda:0")
    side = torch.cuda.Stream()   # where a user's animation kernel would write the records
    res = {}
    for path in ("host", "device"):
        for c in ring:
            if path == "host":
                c.set_instances(inst)
            else:
                c.set_instances_device(words.view(torch.uint8))
        torch.cuda.synchronize()
        pending = [False] * slots
        steps = args.warmup + args.steps
        t0 = None
        for k in range(steps):
            if k == args.warmup:
                for i, c in enumerate(ring):
                    if pending[i]:
                        c.trace_wait(copy=False); pending[i] = False
                t0 = time.perf_counter()
            i = k % slots
            c = ring[i]
            if pending[i]:
                c.trace_wait(copy=False)
            if path == "host":
                c.set_instances(moved(inst, vel, k), update=True)
            else:
                with torch.cuda.stream(side):
                    rec = words.clone()
                    rec[:, 3] += k * vel_t[:, 0]; rec[:, 7] += k * vel_t[:, 1]; rec[:, 11] += k * vel_t[:, 2]
                    c.set_instances_device(rec.view(torch.uint8), update=True, stream=side)
            c.trace_async(W, H)
            pending[i] = True
        for i, c in enumerate(ring):
            if pending[i]:
                c.trace_wait(copy=False)
        res[path] = {"ms_per_step": 1e3 * (time.perf_counter() - t0) / args.steps, "steps": args.steps}
        print("animated, %d instances, %s TLAS: %.3f ms per step" % (n, path, res[path]["ms_per_step"]), flush=True)
    for c in ring[1:]:
        c.close()
    ctx.close()
    res.update({"instances": n, "frame_slots": slots, "frame": [W, H], "max_bounce": 1, "spp": 1})
    return res


def cfg5_static(args, torch):
    w = workloads.make("cfg5", RES)
    ctx = RtContext(0)
    w.apply(ctx)
    W, H = w.width, w.height
    out_t = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    dev = torch.from_numpy(np.ascontiguousarray(w.instances).view(np.uint8).reshape(-1, 64).copy()).to("cuda:0")
    torch.cuda.synchronize()
    ms = {"host": [], "device": []}
    for rnd in range(3):   # alternate the two trees in the same process
        for path in ("host", "device"):
            if path == "host":
                ctx.set_instances(w.instances)
            else:
                ctx.set_instances_device(dev)
            for k in range(args.warmup + args.calls):
                t0 = time.perf_counter()
                ctx.trace_shard(W, H, H, 0, 1, out_t.data_ptr(), out_t.numel() * 4)
                ctx.synchronize()
                if k >= args.warmup:
                    ms[path].append(1e3 * (time.perf_counter() - t0))
    ctx.close()
    res = {p: stats(v) for p, v in ms.items()}
    res["device_over_host"] = res["device"]["median_ms"] / res["host"]["median_ms"]
    print("cfg5 static frame: host SAH TLAS %.3f ms, device LBVH TLAS %.3f ms" % (res["host"]["median_ms"], res["device"]["median_ms"]), flush=True)
    return res


def kernels_only(torch):
    """a few device builds and refits at 16 384 and 262 144 instances for the profiler"""
    for n in (16384, 262144):
        ctx = RtContext(0)
        inst = field(n, seed=n)
        scene(ctx, inst)
        t = torch.from_numpy(inst.view(np.uint8).reshape(-1, 64).copy()).to("cuda:0")
        torch.cuda.synchronize()
        for k in range(6):
            ctx.set_instances_device(t, update=k % 2 == 1)
        ctx.synchronize()
        ctx.close()


def kernel_stats(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r.get("Name", "")
            if any(k in name for k in ("k_inst_records", "k_tlas_", "k_morton", "k_radix_tree", "rocprim")):
                rows.append({k: r[k] for k in r if k in ("Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "Percentage")})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="device_tlas_cost_results.json", help="JSON file to write (default: in the working directory; *_results.json is git-ignored)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="merge the TLAS kernels of a rocprofv3 --stats run under this directory into --out")
    args = ap.parse_args()
    if args.kernel_stats:
        res = json.load(open(args.out)) if os.path.exists(args.out) else {}
        res["kernel_stats"] = kernel_stats(args.kernel_stats)
        json.dump(res, open(args.out, "w"), indent=1)
        print("kernel stats: %d rows" % len(res["kernel_stats"]))
        return
    import torch
    if not torch.cuda.is_available():
        sys.exit("device_tlas_cost.py measures on the GPU: no device")
    if args.kernels_only:
        kernels_only(torch)
        return
    res = {"per_call": per_call(args, torch), "animated": animated(args, torch), "cfg5_static": cfg5_static(args, torch)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
