"""What shading caller-generated rays (rt_shade_rays_device) costs against a frame, on the cfg3 scene at 1920x1080, spp 4, depth 4
(maxBounceCount 3), written to one JSON file.

  pinhole       rt_shade_rays_device on the frame's camera rays: W x H x spp records, sample-major like the frame's sample ids.  The
                per-sample jitter comes from numpy's generator, not from the shader's hash: the same camera, the same distribution of
                directions, not the same bits (the bit-exact pinhole rays are tests/test_shade_rays.py's business).
  fisheye       the same number of rays from the same camera in an equidistant fisheye layout (180 degrees across the image height).
  frame         rt_trace_shard of the frame itself into a device buffer, for comparison.

Each is timed with HIP events around the call on a torch stream: the median of --repeats after --warmup, with per-point averages
(points) and with per-sample colours too (samples).

python3 tools/shade_rays_cost.py --out shade_rays_cost_results.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vulkan_raytracing_amd import RtContext, workloads  # noqa: E402

RES = os.path.join(ROOT, "resources")


def camera(u):
    return [np.asarray(u[f][0][:3], np.float32) for f in ("position", "right", "up", "forward")]


def pinhole_rays(u, W, H, spp, seed=1):
    """src/shader.rgen:62-82 with numpy jitter: d = normalize(ux right + uy up + 2.5 forward), record i * W * H + y * W + x"""
    pos, R, U, F = camera(u)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.zeros((spp, H * W, 8), np.float32)
    for i in range(spp):
        ux = ((x.reshape(-1) + rng.random(H * W)) / W * 2.0 - 1.0).astype(np.float32)
        uy = (1.0 - (y.reshape(-1) + rng.random(H * W)) / H * 2.0).astype(np.float32)
        d = ux[:, None] * R + uy[:, None] * U + np.float32(2.5) * F
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        out[i, :, 0:3] = pos; out[i, :, 4:7] = d; out[i, :, 7] = 10000.0
    return out.reshape(-1, 8)


def fisheye_rays(u, W, H, spp, seed=2):
    """the same camera, equidistant fisheye: theta = pi/2 * r / (H / 2) from the forward axis, r the distance to the image centre"""
    pos, R, U, F = camera(u)
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    out = np.zeros((spp, H * W, 8), np.float32)
    for i in range(spp):
        px = x.reshape(-1) + rng.random(H * W) - W / 2
        py = H / 2 - (y.reshape(-1) + rng.random(H * W))
        r = np.hypot(px, py) / (H / 2)
        th, ph = r * (np.pi / 2), np.arctan2(py, px)
        d = (np.sin(th) * np.cos(ph))[:, None] * R + (np.sin(th) * np.sin(ph))[:, None] * U + np.cos(th)[:, None] * F
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        out[i, :, 0:3] = pos; out[i, :, 4:7] = d; out[i, :, 7] = 10000.0
    return out.reshape(-1, 8)


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max())}


def timed(torch, stream, fn, repeats, warmup):
    out = []
    for i in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            fn()
            e1.record(stream)
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1))
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="shade_rays_cost_results.json")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mesh", default="standin")
    a = ap.parse_args()
    import torch
    wl = workloads.make("cfg3", RES, mesh=a.mesh)
    W, H = wl.width, wl.height
    spp, mb = int(wl.uniforms[0]["samples_per_pixel"]), int(wl.uniforms[0]["max_bounce_count"])
    ctx = RtContext(0)
    wl.apply(ctx)
    stream = torch.cuda.Stream()
    res = {"workload": "cfg3", "mesh": wl.mesh_label, "device": ctx.device_info, "width": W, "height": H, "spp": spp, "depth": mb + 1, "rows": []}
    n_points = W * H
    for kind, make in (("pinhole", pinhole_rays), ("fisheye", fisheye_rays)):
        rays = torch.from_numpy(make(wl.uniforms, W, H, spp)).to("cuda:0")
        srgba = torch.empty((rays.shape[0], 4), dtype=torch.float32, device="cuda:0")
        prgba = torch.empty((n_points, 4), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        for outputs, out in (("points", (None, prgba)), ("samples+points", (srgba, prgba))):
            per_sample = out[0] is not None
            row = {"rays": int(rays.shape[0]), "kind": kind, "outputs": outputs,
                   "device": timed(torch, stream, lambda: ctx.shade_rays_device(rays, samples=spp, per_sample=per_sample, stream=stream, out=out),
                                   a.repeats, a.warmup)}
            p = prgba.cpu().numpy()
            row["points_alpha_1"] = float((p[:, 3] == 1).mean())
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        del rays, srgba
    frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    row = {"rays": n_points * spp, "kind": "frame", "outputs": "rt_trace_shard",
           "device": timed(torch, stream, lambda: ctx.trace_shard(W, H, H, 0, 1, frame.data_ptr(), frame.numel() * 4, stream.cuda_stream),
                           a.repeats, a.warmup)}
    ctx.synchronize()
    res["rows"].append(row)
    print(json.dumps(row), flush=True)
    base = row["device"]["median_ms"]
    for r in res["rows"][:-1]:
        r["vs_frame"] = r["device"]["median_ms"] / base
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
