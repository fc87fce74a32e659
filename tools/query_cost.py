"""What a device ray query (rt_intersect_device) costs against the host entry point (rt_intersect), on the cfg3 scene, written to one
JSON file.

  queries       64 K, 1 M and 8 M rays; camera-coherent primary rays (one per pixel, scanline order) and incoherent random rays;
                closest hit, closest hit with attributes, any hit.  device_ms: HIP events around the query on a torch stream (median
                of --repeats after --warmup); host_ms: host clock around rt_intersect from host rays to host hits (it blocks).
  in_flight     the same 1 M-ray queries while 4 frame slots each render a cfg3 frame (rt_trace_async): the device query runs beside
                the frames (frames_with_query_ms: the 4 frames and the query, host clock); rt_intersect refuses a context with a pending
                rt_trace_async frame, so it runs on slot 0 beside the frames of the other three.  frames_alone: the 4 frames, for scale.

python3 tools/query_cost.py --out query_cost_results.json"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vulkan_raytracing_amd import RtContext, workloads  # noqa: E402

RES = os.path.join(ROOT, "resources")
SIZES = [64 << 10, 1 << 20, 8 << 20]
MODES = {"closest": dict(any_hit=False), "closest_attr": dict(any_hit=False, attributes=True), "any": dict(any_hit=True)}


def primary_rays(u, n):
    """n camera rays of the cfg3 camera (src/shader.rgen:74-79: direction ux right + uy up + 2.5 forward), one per pixel of a
    16:9 image with about n pixels, in scanline order"""
    h = int(np.sqrt(n * 9 / 16))
    w = (n + h - 1) // h
    k = np.arange(n)
    ux = ((k % w) + 0.5) / w * 2.0 - 1.0
    uy = 1.0 - ((k // w) + 0.5) / h * 2.0
    ux = ux * (w / h)
    R, U, F = (np.asarray(u[f][0][:3], np.float64) for f in ("right", "up", "forward"))
    d = ux[:, None] * R + uy[:, None] * U + 2.5 * F
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = np.asarray(u["position"][0][:3], np.float32)
    r[:, 3] = 0.001; r[:, 4:7] = d; r[:, 7] = 10000.0
    return r


def random_rays(n, seed=1):
    """incoherent rays: origins in a ball of radius 20 about the scene, directions towards random points of a ball of radius 4"""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(n, 3)).astype(np.float32); o *= 20.0 * rng.uniform(0.3, 1.0, (n, 1)).astype(np.float32) / np.linalg.norm(o, axis=1, keepdims=True)
    t = rng.normal(size=(n, 3)).astype(np.float32) * 2.0
    d = t - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = o; r[:, 3] = 0.001; r[:, 4:7] = d; r[:, 7] = 10000.0
    return r


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max())}


def device_ms(torch, ctx, rays, kw, stream, repeats, warmup):
    out = []
    for i in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            ctx.intersect_device(rays, stream=stream, **kw)
            e1.record(stream)
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


def host_ms(ctx, rays, any_hit, repeats, warmup):
    out = []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        ctx.intersect(rays, any_hit=any_hit)
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="query_cost_results.json")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--mesh", default="standin")
    a = ap.parse_args()
    import torch
    wl = workloads.make("cfg3", RES, mesh=a.mesh)
    ctx = RtContext(0)
    slots = [ctx] + [ctx.frame_slot() for _ in range(3)]
    wl.apply(ctx)
    for s in slots[1:]:
        s.set_instances(wl.instances)
        s.set_uniforms(wl.uniforms)
    stream = torch.cuda.Stream()
    res = {"workload": "cfg3", "mesh": wl.mesh_label, "device": ctx.device_info, "queries": [], "in_flight": {}}
    for n in SIZES:
        for kind in ("primary", "random"):
            rays_np = primary_rays(wl.uniforms, n) if kind == "primary" else random_rays(n)
            rays = torch.from_numpy(rays_np).to("cuda:0")
            torch.cuda.synchronize()
            for mode, kw in MODES.items():
                row = {"rays": n, "kind": kind, "mode": mode,
                       "device": stats(device_ms(torch, ctx, rays, kw, stream, a.repeats, a.warmup))}
                if mode != "closest_attr":
                    row["host_rt_intersect"] = stats(host_ms(ctx, rays_np, kw["any_hit"], a.host_repeats, 1))
                    row["speedup_median"] = row["host_rt_intersect"]["median_ms"] / row["device"]["median_ms"]
                res["queries"].append(row)
                print(json.dumps(row), flush=True)
            del rays
    # 4 frame slots rendering at the same time
    W, H = wl.width, wl.height
    for s in slots:
        s.trace(W, H)
    t = []
    for _ in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        for s in slots:
            s.trace_async(W, H)
        for s in slots:
            s.trace_wait(copy=False)
        t.append((time.perf_counter() - t0) * 1e3)
    res["in_flight"]["frames_alone_4_slots_ms"] = stats(t[a.warmup:])
    n = 1 << 20
    for kind in ("primary", "random"):
        rays_np = primary_rays(wl.uniforms, n) if kind == "primary" else random_rays(n)
        rays = torch.from_numpy(rays_np).to("cuda:0")
        torch.cuda.synchronize()
        dq, hq, fr = [], [], []
        for i in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            for s in slots:
                s.trace_async(W, H)
            ms = device_ms(torch, ctx, rays, {}, stream, 1, 0)
            for s in slots:
                s.trace_wait(copy=False)
            if i >= a.warmup:
                dq += ms
                fr.append((time.perf_counter() - t0) * 1e3)
        # rt_intersect refuses a context whose rt_trace_async frame is pending, and waits for one of rt_trace_shard: it runs on
        # slot 0 beside the frames of the other three slots
        for i in range(a.host_repeats + 1):
            for s in slots[1:]:
                s.trace_async(W, H)
            t0 = time.perf_counter()
            ctx.intersect(rays_np)
            if i:
                hq.append((time.perf_counter() - t0) * 1e3)
            for s in slots[1:]:
                s.trace_wait(copy=False)
        res["in_flight"][kind] = {"rays": n, "device_query_beside_4_frames": stats(dq), "frames_with_query_ms": stats(fr),
                                  "host_rt_intersect_beside_3_frames": stats(hq)}
        print(json.dumps({kind: res["in_flight"][kind]}), flush=True)
    for s in reversed(slots):
        s.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
