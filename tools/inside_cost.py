"""What the inside / outside vote (rt_point_inside_device) and the signed distance (rt_signed_distance_device) cost on the cfg3 scene
(teapot + stand-in), beside what a torch user composes from the all-hits count query today, written to one JSON file.

  points        --points records (default 1 M) uniform in the scene's box, r_max = inf.
  device_ms     HIP events around the call on a torch stream: the median of --repeats calls after --warmup calls; the four forms
                take turns within every repeat.
  (a) inside    point_inside_device(n_dirs=3): no ray-sized data, early stop.
  (b) composed  torch builds the 3 x points rays (o, 0, D_k, inf), intersect_device_hits(rays, 0) counts them, torch takes the
                parities and the majority: all of it inside the timed window.
  (c) closest   closest_point_device alone.
  (d) signed    signed_distance_device(n_dirs=3).
  also          point_inside_device with counts (no early stop) and with 1 and 5 directions; per point the node visits and triangle
                tests of the host form with counting, on the first --count-points records, for 1, 3 and 5 directions; the share of
                points inside and of points decided after two directions.

python3 tools/inside_cost.py --out inside_cost_results.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.closest_point_cost import stats, world_triangles  # noqa: E402
from vulkan_raytracing_amd import RtContext, api, workloads  # noqa: E402

RES = os.path.join(ROOT, "resources")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="inside_cost_results.json")
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
    A, B, C = world_triangles(wl)
    P = np.concatenate([A, B, C])
    lo, hi = P.min(axis=0), P.max(axis=0)
    rng = np.random.default_rng(1)
    n = a.points
    pts_np = np.concatenate([lo + rng.uniform(size=(n, 3)) * (hi - lo), np.full((n, 1), np.inf)], axis=1).astype(np.float32)
    pts = torch.from_numpy(pts_np).to("cuda:0")
    dirs = torch.tensor(api.INSIDE_DIRS[:3], dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def composed(s):
        rays = torch.zeros((n, 3, 8), dtype=torch.float32, device="cuda:0")
        rays[:, :, 0:3] = pts[:, None, 0:3]
        rays[:, :, 4:7] = dirs[None, :, :]
        rays[:, :, 7] = float("inf")
        cnt = ctx.intersect_device_hits(rays.view(-1, 8), 0, stream=s).count.view(n, 3)
        return (cnt & 1).sum(dim=1) >= 2

    forms = {"inside": lambda s: ctx.point_inside_device(pts, n_dirs=3, stream=s),
             "composed": composed,
             "closest": lambda s: ctx.closest_point_device(pts, stream=s),
             "signed": lambda s: ctx.signed_distance_device(pts, n_dirs=3, stream=s),
             "inside_counts": lambda s: ctx.point_inside_device(pts, n_dirs=3, counts=True, stream=s),
             "inside_1": lambda s: ctx.point_inside_device(pts, n_dirs=1, stream=s),
             "inside_5": lambda s: ctx.point_inside_device(pts, n_dirs=5, stream=s)}
    ms = {k: [] for k in forms}
    for i in range(a.warmup + a.repeats):
        for k, call in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                call(stream)
                e1.record(stream)
            e1.synchronize()
            if i >= a.warmup:
                ms[k].append(e0.elapsed_time(e1))
    res = {"workload": "cfg3", "mesh": wl.mesh_label, "device": ctx.device_info, "triangles": int(len(A)), "points": n,
           "device_ms": {k: stats(v) for k, v in ms.items()}}
    print(json.dumps(res["device_ms"]), flush=True)
    # the two forms agree
    with torch.cuda.stream(stream):
        w = ctx.point_inside_device(pts, n_dirs=3, stream=stream).word
        same = bool((((w & 1) != 0) == composed(stream)).all().item())
        taken = (w >> 16) & 0xFF
        res["agree_with_composed"] = same
        res["inside_share"] = float((w & 1).float().mean().item())
        res["decided_after_two"] = float((taken == 2).float().mean().item())
    stream.synchronize()
    m = min(a.count_points, n)
    res["per_point"] = {}
    for k in (1, 3, 5):
        _, _, st = ctx.point_inside(pts_np[:m], n_dirs=k, counting=True)
        res["per_point"][str(k)] = {"node_visits": st.node_visits / m, "tri_tests": st.tri_tests / m}
    _, _, st = ctx.point_inside(pts_np[:m], n_dirs=3, counts=True, counting=True)
    res["per_point"]["3_all_directions"] = {"node_visits": st.node_visits / m, "tri_tests": st.tri_tests / m}
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "device_ms"}))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
