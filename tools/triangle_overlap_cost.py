"""What a triangle-overlap query (rt_overlap_triangles_device) costs on the cfg3 scene (teapot + stand-in), beside the box-overlap query
(rt_overlap_boxes_device) on the same queries' bounding boxes, written to one JSON file.  The two walks visit the same nodes and
packets (the node test is the same), so their ratio is the price of the seventeen-axis leaf test over the thirteen-axis one.

  query sets    (a) triangles of 0.1 % to 1 % of the scene diagonal around surface samples; (b) triangles of 1 % to 10 % of the diagonal
                uniform in the scene box.  --queries each (default 1 M).
  modes         count (max_ids 0), ids (max_ids 16 with counts), ids without counts (the pruning walk), any (RT_OVERLAP_ANY).
  device_ms     HIP events around the call on a torch stream; the triangle and the box query take turns (t, b, t, b, ...): the median
                of --repeats calls of each after --warmup calls of each.
  per query     node_visits and tri_tests of both host forms with counting, on the first --count-queries records, and the candidates.

python3 tools/triangle_overlap_cost.py --out triangle_overlap_cost_results.json"""
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


def query_sets(tris, n, seed=1):
    A, B, C = tris
    rng = np.random.default_rng(seed)
    P = np.concatenate([A, B, C])
    lo, hi = P.min(axis=0), P.max(axis=0)
    diag = float(np.linalg.norm(hi - lo))
    k = rng.integers(0, len(A), n)
    u, v = rng.uniform(size=n), rng.uniform(size=n)
    fl = u + v > 1
    u, v = np.where(fl, 1 - u, u), np.where(fl, 1 - v, v)
    pa = A[k] + u[:, None] * (B[k] - A[k]) + v[:, None] * (C[k] - A[k])
    pb = lo + rng.uniform(size=(n, 3)) * (hi - lo)

    def rec(c, h):
        w = rng.normal(size=(n, 3, 3))
        w -= w.mean(axis=1, keepdims=True)
        w /= np.abs(w).max(axis=(1, 2), keepdims=True)
        q = np.zeros((n, 3, 4), np.float32)
        q[:, :, :3] = c[:, None] + h[:, :, None] * w      # (the bounds are about 2 h wide)
        return q.reshape(n, 12)
    return {"a": rec(pa, 0.5 * diag * 10 ** rng.uniform(-3, -2, (n, 1))), "b": rec(pb, 0.5 * diag * 10 ** rng.uniform(-2, -1, (n, 1)))}, diag


def bounds(q):
    P = q.reshape(-1, 3, 4)[:, :, :3]
    b = np.zeros((len(q), 8), np.float32)
    b[:, 0:3] = P.min(axis=1); b[:, 4:7] = P.max(axis=1)
    return b


def alternated(torch, calls, stream, repeats, warmup):
    """the calls take turns; returns one list of milliseconds per call"""
    out = [[] for _ in calls]
    for i in range(warmup + repeats):
        for j, call in enumerate(calls):
            ms = timed(torch, call, stream, 1, 0)
            if i >= warmup:
                out[j] += ms
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="triangle_overlap_cost_results.json")
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--count-queries", type=int, default=1 << 18)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mesh", default="standin")
    a = ap.parse_args()
    import torch
    wl = workloads.make("cfg3", RES, mesh=a.mesh)
    ctx = RtContext(0)
    wl.apply(ctx)
    tris = world_triangles(wl)
    sets, diag = query_sets(tris, a.queries)
    stream = torch.cuda.Stream()
    res = {"workload": "cfg3", "mesh": wl.mesh_label, "device": ctx.device_info, "triangles": int(len(tris[0])), "queries": a.queries, "diagonal": diag, "sets": []}
    modes = {"count": dict(max_ids=0), "ids16": dict(max_ids=16), "ids16_no_counts": dict(max_ids=16, counts=False), "any": dict(max_ids=0, any=True)}
    for name, q_np in sets.items():
        b_np = bounds(q_np)
        q, b = torch.from_numpy(q_np).to("cuda:0"), torch.from_numpy(b_np).to("cuda:0")
        torch.cuda.synchronize()
        row = {"set": name}
        for mode, kw in modes.items():
            t_ms, b_ms = alternated(torch, [lambda s: ctx.overlap_triangles_device(q, stream=s, **kw), lambda s: ctx.overlap_boxes_device(b, stream=s, **kw)],
                                    stream, a.repeats, a.warmup)
            row[mode] = {"triangles": stats(t_ms), "boxes": stats(b_ms), "ratio": float(np.median(t_ms) / np.median(b_ms))}
        m = min(a.count_queries, a.queries)
        tc, _, ts = ctx.overlap_triangles(q_np[:m], counting=True)
        bc, _, bs = ctx.overlap_boxes(b_np[:m], counting=True)
        row["node_visits_per_query"] = {"triangles": ts.node_visits / m, "boxes": bs.node_visits / m}
        row["tri_tests_per_query"] = {"triangles": ts.tri_tests / m, "boxes": bs.tri_tests / m}
        row["candidates_per_query"] = {"triangles": float(tc.mean()), "boxes": float(bc.mean())}
        row["hit_share"] = {"triangles": float((tc > 0).mean()), "boxes": float((bc > 0).mean())}
        res["sets"].append(row)
        print(json.dumps(row), flush=True)
        del q, b
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
