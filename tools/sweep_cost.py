"""What a sphere sweep (rt_sweep_spheres_device) costs on the cfg3 scene (teapot + stand-in), beside the closest-hit ray query
(rt_intersect_device) on the same rays, written to one JSON file.

  sweeps        --sweeps records (default 1 M) from outside the scene box towards surface samples, tmax = inf, the same origins and
                directions at every radius: 0, 1e-3, 1e-2 and 1e-1 of the scene extent (the longest side of its box).
  device_ms     HIP events around the call on a torch stream: the median of --repeats calls after --warmup calls.
  closest_hit   rt_intersect_device on the same origins and directions (tmin = 0), timed the same way in the same run.
  per sweep     node_visits and tri_tests of the host form with counting (rt_sweep_spheres), on the first --count-sweeps records.

python3 tools/sweep_cost.py --out sweep_cost_results.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.closest_point_cost import stats, timed, world_triangles  # noqa: E402
from vulkan_raytracing_amd import RtContext, workloads  # noqa: E402

RES = os.path.join(ROOT, "resources")


def aimed_rays(tris, n, seed=1):
    """(origins, unit directions, extent): from a sphere of 0.8 to 1.5 diagonals around the scene towards uniform surface samples"""
    A, B, C = tris
    rng = np.random.default_rng(seed)
    P = np.concatenate([A, B, C])
    lo, hi = P.min(axis=0), P.max(axis=0)
    c, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    k = rng.integers(0, len(A), n)
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    fl = u + v > 1
    u, v = np.where(fl, 1 - u, u), np.where(fl, 1 - v, v)
    tgt = A[k] + u[:, None] * (B[k] - A[k]) + v[:, None] * (C[k] - A[k])
    o = rng.normal(size=(n, 3)); o /= np.linalg.norm(o, axis=1, keepdims=True)
    o = c + o * diag * rng.uniform(0.8, 1.5, (n, 1))
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d, float((hi - lo).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="sweep_cost_results.json")
    ap.add_argument("--sweeps", type=int, default=1 << 20)
    ap.add_argument("--count-sweeps", type=int, default=1 << 18)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mesh", default="standin")
    a = ap.parse_args()
    import torch
    wl = workloads.make("cfg3", RES, mesh=a.mesh)
    ctx = RtContext(0)
    wl.apply(ctx)
    tris = world_triangles(wl)
    o, d, ext = aimed_rays(tris, a.sweeps)
    rec = np.zeros((a.sweeps, 8), np.float32)
    rec[:, 0:3] = o; rec[:, 4:7] = d
    stream = torch.cuda.Stream()
    res = {"workload": "cfg3", "mesh": wl.mesh_label, "device": ctx.device_info, "triangles": int(len(tris[0])), "sweeps": a.sweeps, "extent": ext, "radii": []}
    rays_np = rec.copy(); rays_np[:, 7] = 1e6
    rays = torch.from_numpy(rays_np).to("cuda:0")
    torch.cuda.synchronize()
    res["closest_hit"] = stats(timed(torch, lambda s: ctx.intersect_device(rays, stream=s), stream, a.repeats, a.warmup))
    print(json.dumps({"closest_hit": res["closest_hit"]}), flush=True)
    m = min(a.count_sweeps, a.sweeps)
    for f in (0.0, 1e-3, 1e-2, 1e-1):
        sw_np = rec.copy(); sw_np[:, 3] = f * ext; sw_np[:, 7] = np.inf
        sw = torch.from_numpy(sw_np).to("cuda:0")
        torch.cuda.synchronize()
        row = {"radius_of_extent": f,
               "sweep": stats(timed(torch, lambda s: ctx.sweep_spheres_device(sw, stream=s), stream, a.repeats, a.warmup)),
               "sweep_attr": stats(timed(torch, lambda s: ctx.sweep_spheres_device(sw, attributes=True, stream=s), stream, a.repeats, a.warmup)),
               "closest_hit": stats(timed(torch, lambda s: ctx.intersect_device(rays, stream=s), stream, a.repeats, a.warmup))}
        h, st = ctx.sweep_spheres(sw_np[:m], counting=True)
        row["node_visits_per_sweep"] = st.node_visits / m
        row["tri_tests_per_sweep"] = st.tri_tests / m
        row["found"] = float((h["inst"] >= 0).mean())
        res["radii"].append(row)
        print(json.dumps(row), flush=True)
        del sw
    hr, st = ctx.intersect(rays_np[:m], counting=True)
    res["closest_hit_node_visits_per_ray"] = st.node_visits / m
    res["closest_hit_tri_tests_per_ray"] = st.tri_tests / m
    res["closest_hit_found"] = float((hr["inst"] >= 0).mean())
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
