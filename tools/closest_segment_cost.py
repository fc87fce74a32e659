"""What a closest-segment query (rt_closest_segment_device) costs on the cfg3 scene (teapot + stand-in), beside the closest-point query
(rt_closest_point_device) on the segments' midpoints, written to one JSON file.

  segment sets  P0 a surface sample displaced by up to 1 % of the scene diagonal, P1 = P0 + L diag u for a random unit u, with
                L = 0.01, 0.1 and 1 (--lengths); r_max = inf.  --segments each (default 1 M).
  device_ms     HIP events around the call on a torch stream: the median of --repeats calls after --warmup calls.
  closest_point rt_closest_point_device on the midpoints (r_max = inf), timed the same way.
  per record    node_visits and tri_tests of the host forms with counting (rt_closest_segment, rt_closest_point), on the first
                --count-segments records.

The walk's second node test (csrc/kernels_segment.inc, RT_SEGMENT_SLAB) is a compile-time choice: build the library without it with
`make exp EXP_NAME=noslab EXP_FLAGS=-DRT_SEGMENT_SLAB=0` and run this tool again with --variant noslab.

python3 tools/closest_segment_cost.py --out closest_segment_cost_results.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.closest_point_cost import stats, timed, world_triangles  # noqa: E402
from vulkan_raytracing_amd import RtContext, api, workloads  # noqa: E402

RES = os.path.join(ROOT, "resources")


def segment_sets(tris, n, lengths, seed=1):
    A, B, C = tris
    rng = np.random.default_rng(seed)
    P = np.concatenate([A, B, C])
    lo, hi = P.min(axis=0), P.max(axis=0)
    diag = float(np.linalg.norm(hi - lo))
    k = rng.integers(0, len(A), n)
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    fl = u + v > 1
    u, v = np.where(fl, 1 - u, u), np.where(fl, 1 - v, v)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    p0 = A[k] + u[:, None] * (B[k] - A[k]) + v[:, None] * (C[k] - A[k]) + d * rng.uniform(0, 0.01 * diag, (n, 1))
    w = rng.normal(size=(n, 3)); w /= np.linalg.norm(w, axis=1, keepdims=True)
    return {L: api.capsule_records(p0, p0 + L * diag * w, np.inf) for L in lengths}, diag


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="closest_segment_cost_results.json")
    ap.add_argument("--segments", type=int, default=1 << 20)
    ap.add_argument("--count-segments", type=int, default=1 << 18)
    ap.add_argument("--lengths", type=float, nargs="+", default=[0.01, 0.1, 1.0])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mesh", default="standin")
    ap.add_argument("--variant", default=None, help="librt_mi355x_<variant>.so (see the module's text)")
    a = ap.parse_args()
    import torch
    wl = workloads.make("cfg3", RES, mesh=a.mesh)
    ctx = RtContext(0, variant=a.variant)
    wl.apply(ctx)
    tris = world_triangles(wl)
    sets, diag = segment_sets(tris, a.segments, a.lengths)
    stream = torch.cuda.Stream()
    res = {"workload": "cfg3", "mesh": wl.mesh_label, "device": ctx.device_info, "variant": a.variant or "product", "triangles": int(len(tris[0])),
           "segments": a.segments, "diagonal": diag, "sets": []}
    for L, segs_np in sets.items():
        mid_np = np.concatenate([(segs_np[:, 0:3].astype(np.float64) + segs_np[:, 4:7]) / 2, np.full((a.segments, 1), np.inf)], axis=1).astype(np.float32)
        segs, mid = torch.from_numpy(segs_np).to("cuda:0"), torch.from_numpy(mid_np).to("cuda:0")
        torch.cuda.synchronize()
        row = {"length_diagonals": L,
               "closest_segment": stats(timed(torch, lambda s: ctx.closest_segment_device(segs, stream=s), stream, a.repeats, a.warmup)),
               "closest_segment_attr": stats(timed(torch, lambda s: ctx.closest_segment_device(segs, attributes=True, params=True, stream=s), stream, a.repeats,
                                                   a.warmup)),
               "closest_point_midpoints": stats(timed(torch, lambda s: ctx.closest_point_device(mid, stream=s), stream, a.repeats, a.warmup))}
        m = min(a.count_segments, a.segments)
        h, st = ctx.closest_segment(segs_np[:m], counting=True)
        row["node_visits_per_segment"] = st.node_visits / m
        row["tri_tests_per_segment"] = st.tri_tests / m
        row["touching"] = float((h["t"] <= 1e-6 * diag).mean())
        _, st = ctx.closest_point(mid_np[:m], counting=True)
        row["node_visits_per_midpoint"] = st.node_visits / m
        row["tri_tests_per_midpoint"] = st.tri_tests / m
        res["sets"].append(row)
        print(json.dumps(row), flush=True)
        del segs, mid
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
