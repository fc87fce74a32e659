"""What a closest-triangle query (rt_closest_triangle_device) costs on the cfg3 scene (teapot + stand-in), beside three closest-segment
records per triangle (rt_closest_segment_device on its edges: the nearest existing composition, which answers a weaker question and
serves as a scale, not a target), written to one JSON file.

  triangle sets  P0 a surface sample displaced by up to 1 % of the scene diagonal, P1 and P2 = P0 + S diag u for two random unit u:
                 cloth-sized (S = 0.005, --triangles records, default 1 M), link-sized (S = 0.05, a quarter of that) and scene-spanning
                 (S = 0.5, a sixty-fourth); r_max = inf.
  device_ms      HIP events around the call on a torch stream: the median of --repeats calls after --warmup calls; records_per_s from it.
  edges          rt_closest_segment_device on the 3 n edge records in one call, timed the same way.
  per record     node_visits and tri_tests of the host forms with counting (rt_closest_triangle, rt_closest_segment), on the first
                 --count-triangles records.

The walk's second node test (csrc/kernels_triangle.inc, RT_TRIANGLE_PLANE) is a compile-time choice: build the library with the other
setting with `make exp EXP_NAME=noplane EXP_FLAGS=-DRT_TRIANGLE_PLANE=0` (or =1 as EXP_NAME=plane) and run this tool again with
--variant noplane (plane).

python3 tools/closest_triangle_cost.py --out closest_triangle_cost_results.json"""
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
SETS = (("cloth", 0.005, 1), ("link", 0.05, 4), ("spanning", 0.5, 64))   # name, size in diagonals, divisor of --triangles


def triangle_set(tris, n, size, seed):
    A, B, C = tris
    rng = np.random.default_rng(seed)
    P = np.concatenate([A, B, C])
    diag = float(np.linalg.norm(P.max(axis=0) - P.min(axis=0)))
    k = rng.integers(0, len(A), n)
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    fl = u + v > 1
    u, v = np.where(fl, 1 - u, u), np.where(fl, 1 - v, v)

    def unit():
        d = rng.normal(size=(n, 3))
        return d / np.linalg.norm(d, axis=1, keepdims=True)
    p0 = A[k] + u[:, None] * (B[k] - A[k]) + v[:, None] * (C[k] - A[k]) + unit() * rng.uniform(0, 0.01 * diag, (n, 1))
    rec = np.zeros((n, 12), np.float32)
    rec[:, 0:3] = p0; rec[:, 3] = np.inf
    rec[:, 4:7] = p0 + size * diag * unit(); rec[:, 8:11] = p0 + size * diag * unit()
    return rec, diag


def edge_records(rec):
    out = np.zeros((3, len(rec), 8), np.float32)
    for e, (i, j) in enumerate(((0, 1), (1, 2), (2, 0))):
        out[e, :, 0:3] = rec[:, 4 * i:4 * i + 3]; out[e, :, 3] = rec[:, 3]; out[e, :, 4:7] = rec[:, 4 * j:4 * j + 3]
    return out.reshape(-1, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="closest_triangle_cost_results.json")
    ap.add_argument("--triangles", type=int, default=1 << 20)
    ap.add_argument("--count-triangles", type=int, default=1 << 16)
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
    stream = torch.cuda.Stream()
    res = {"workload": "cfg3", "mesh": wl.mesh_label, "device": ctx.device_info, "variant": a.variant or "product", "triangles": int(len(tris[0])), "sets": []}
    for seed, (name, size, div) in enumerate(SETS):
        n = max(1, a.triangles // div)
        rec_np, diag = triangle_set(tris, n, size, seed + 1)
        seg_np = edge_records(rec_np)
        rec, seg = torch.from_numpy(rec_np).to("cuda:0"), torch.from_numpy(seg_np).to("cuda:0")
        torch.cuda.synchronize()
        row = {"set": name, "size_diagonals": size, "records": n, "diagonal": diag,
               "closest_triangle": stats(timed(torch, lambda s: ctx.closest_triangle_device(rec, stream=s), stream, a.repeats, a.warmup)),
               "closest_triangle_attr": stats(timed(torch, lambda s: ctx.closest_triangle_device(rec, attributes=True, params=True, stream=s), stream, a.repeats,
                                                    a.warmup)),
               "closest_segment_3_edges": stats(timed(torch, lambda s: ctx.closest_segment_device(seg, stream=s), stream, a.repeats, a.warmup))}
        row["records_per_s"] = n / (row["closest_triangle"]["median_ms"] * 1e-3)
        m = min(a.count_triangles, n)
        h, st = ctx.closest_triangle(rec_np[:m], counting=True)
        row["node_visits_per_triangle"] = st.node_visits / m
        row["tri_tests_per_triangle"] = st.tri_tests / m
        row["touching"] = float((h["t"] <= 1e-6 * diag).mean())
        _, st = ctx.closest_segment(seg_np.reshape(3, n, 8)[:, :m].reshape(-1, 8), counting=True)
        row["node_visits_per_3_edges"] = st.node_visits / m
        row["tri_tests_per_3_edges"] = st.tri_tests / m
        res["sets"].append(row)
        print(json.dumps(row), flush=True)
        del rec, seg
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
