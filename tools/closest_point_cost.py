"""What a closest-point query (rt_closest_point_device) costs on the cfg3 scene (teapot + stand-in), beside the closest-hit ray query
(rt_intersect_device) for the same number of records, written to one JSON file.

  point sets    (a) surface samples displaced by up to 1 % of the scene diagonal; (b) points uniform in twice the scene box;
                (c) set (b) with r_max = 1 % of the diagonal.  --points each (default 1 M).
  device_ms     HIP events around the call on a torch stream: the median of --repeats calls after --warmup calls.
  closest_hit   rt_intersect_device on rays from the same points in random directions, timed the same way.
  per point     node_visits and tri_tests of the host form with counting (rt_closest_point), on the first --count-points records.

python3 tools/closest_point_cost.py --out closest_point_cost_results.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vulkan_raytracing_amd import RtContext, workloads  # noqa: E402

RES = os.path.join(ROOT, "resources")


def world_triangles(wl):
    """(A, B, C) world vertices of every triangle of every instance, binary64"""
    g = wl.geometry
    verts = np.asarray(g.verts, np.float32).reshape(-1)
    idx = np.asarray(g.idx, np.int64)
    out = []
    for r in wl.instances:
        ff, fi, pc = g.ranges[int(r["mesh"])]
        ix = idx[fi:fi + 3 * pc].reshape(-1, 3)
        p = verts[ff:].reshape(-1, 6)[:, :3].astype(np.float64)
        M = np.asarray(r["transform"], np.float64).reshape(3, 4)
        w = p @ M[:, :3].T + M[:, 3]
        out.append((w[ix[:, 0]], w[ix[:, 1]], w[ix[:, 2]]))
    return tuple(np.concatenate([o[k] for o in out]) for k in range(3))


def point_sets(tris, n, seed=1):
    A, B, C = tris
    rng = np.random.default_rng(seed)
    P = np.concatenate([A, B, C])
    lo, hi = P.min(axis=0), P.max(axis=0)
    c, diag = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    k = rng.integers(0, len(A), n)
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    fl = u + v > 1
    u, v = np.where(fl, 1 - u, u), np.where(fl, 1 - v, v)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    a = A[k] + u[:, None] * (B[k] - A[k]) + v[:, None] * (C[k] - A[k]) + d * rng.uniform(0, 0.01 * diag, (n, 1))
    b = c + rng.uniform(-1, 1, (n, 3)) * (hi - lo)

    def rec(p, r):
        return np.concatenate([p, np.full((n, 1), r)], axis=1).astype(np.float32)
    return {"a": rec(a, np.inf), "b": rec(b, np.inf), "c": rec(b, 0.01 * diag)}, diag


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": float(np.median(a)), "min_ms": float(a.min()), "max_ms": float(a.max())}


def timed(torch, call, stream, repeats, warmup):
    out = []
    for i in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            call(stream)
            e1.record(stream)
        e1.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="closest_point_cost_results.json")
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--count-points", type=int, default=1 << 18)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mesh", default="standin")
    a = ap.parse_args()
    import torch
    wl = workloads.make("cfg3", RES, mesh=a.mesh)
    ctx = RtContext(0)
    wl.apply(ctx)
    tris = world_triangles(wl)
    sets, diag = point_sets(tris, a.points)
    stream = torch.cuda.Stream()
    res = {"workload": "cfg3", "mesh": wl.mesh_label, "device": ctx.device_info, "triangles": int(len(tris[0])), "points": a.points, "diagonal": diag, "sets": []}
    rng = np.random.default_rng(2)
    for name, pts_np in sets.items():
        pts = torch.from_numpy(pts_np).to("cuda:0")
        d = rng.normal(size=(a.points, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays_np = np.zeros((a.points, 8), np.float32)
        rays_np[:, 0:3] = pts_np[:, :3]; rays_np[:, 3] = 0.0; rays_np[:, 4:7] = d; rays_np[:, 7] = 1e4
        rays = torch.from_numpy(rays_np).to("cuda:0")
        torch.cuda.synchronize()
        row = {"set": name,
               "closest_point": stats(timed(torch, lambda s: ctx.closest_point_device(pts, stream=s), stream, a.repeats, a.warmup)),
               "closest_point_attr": stats(timed(torch, lambda s: ctx.closest_point_device(pts, attributes=True, stream=s), stream, a.repeats, a.warmup)),
               "closest_hit": stats(timed(torch, lambda s: ctx.intersect_device(rays, stream=s), stream, a.repeats, a.warmup))}
        m = min(a.count_points, a.points)
        h, st = ctx.closest_point(pts_np[:m], counting=True)
        row["node_visits_per_point"] = st.node_visits / m
        row["tri_tests_per_point"] = st.tri_tests / m
        row["found"] = float((h["inst"] >= 0).mean())
        res["sets"].append(row)
        print(json.dumps(row), flush=True)
        del pts, rays
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
