"""What a box-overlap query (rt_overlap_boxes_device) costs on the cfg3 scene (teapot + stand-in), beside the closest-point query
(rt_closest_point_device) for the same number of records, written to one JSON file.

  box sets      (a) boxes of 0.1 % to 1 % of the scene diagonal centred on surface samples; (b) boxes of 1 % to 10 % of the diagonal
                uniform in the scene box.  --boxes each (default 1 M).
  modes         count (max_ids 0), ids (max_ids 16 with counts), ids without counts (the pruning walk), any (RT_OVERLAP_ANY).
  device_ms     HIP events around the call on a torch stream: the median of --repeats calls after --warmup calls.
  closest_point rt_closest_point_device on the boxes' centres with r_max = inf, timed the same way.
  per box       node_visits and tri_tests of the host form with counting (rt_overlap_boxes), on the first --count-boxes records.
  voxel grid    --grid^3 (default 256) voxels over the scene box: count mode against RT_OVERLAP_ANY, and the occupied share.

python3 tools/overlap_cost.py --out overlap_cost_results.json"""
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


def box_sets(tris, n, seed=1):
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
        b = np.zeros((n, 8), np.float32)
        b[:, 0:3] = c - h; b[:, 4:7] = c + h
        return b
    return {"a": rec(pa, 0.5 * diag * 10 ** rng.uniform(-3, -2, (n, 1))), "b": rec(pb, 0.5 * diag * 10 ** rng.uniform(-2, -1, (n, 1)))}, (lo, hi, diag)


def voxel_grid(torch, lo, hi, g):
    """g^3 voxels over [lo, hi] as an (g^3, 8) float32 tensor on the GPU"""
    t = torch.arange(g, dtype=torch.float64, device="cuda:0")
    x, y, z = torch.meshgrid(t, t, t, indexing="ij")
    ijk = torch.stack([x, y, z], dim=-1).reshape(-1, 3)
    lo_t, cell = torch.tensor(lo, dtype=torch.float64, device="cuda:0"), torch.tensor((hi - lo) / g, dtype=torch.float64, device="cuda:0")
    b = torch.zeros((g ** 3, 8), dtype=torch.float32, device="cuda:0")
    b[:, 0:3] = (lo_t + ijk * cell).to(torch.float32)
    b[:, 4:7] = (lo_t + (ijk + 1) * cell).to(torch.float32)
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="overlap_cost_results.json")
    ap.add_argument("--boxes", type=int, default=1 << 20)
    ap.add_argument("--count-boxes", type=int, default=1 << 18)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mesh", default="standin")
    a = ap.parse_args()
    import torch
    wl = workloads.make("cfg3", RES, mesh=a.mesh)
    ctx = RtContext(0)
    wl.apply(ctx)
    tris = world_triangles(wl)
    sets, (lo, hi, diag) = box_sets(tris, a.boxes)
    stream = torch.cuda.Stream()
    res = {"workload": "cfg3", "mesh": wl.mesh_label, "device": ctx.device_info, "triangles": int(len(tris[0])), "boxes": a.boxes, "diagonal": diag, "sets": []}
    modes = {"count": dict(max_ids=0), "ids16": dict(max_ids=16), "ids16_no_counts": dict(max_ids=16, counts=False), "any": dict(max_ids=0, any=True)}
    for name, b_np in sets.items():
        boxes = torch.from_numpy(b_np).to("cuda:0")
        pts_np = np.concatenate([(b_np[:, 0:3] + b_np[:, 4:7]) / 2, np.full((a.boxes, 1), np.inf, np.float32)], axis=1).astype(np.float32)
        pts = torch.from_numpy(pts_np).to("cuda:0")
        torch.cuda.synchronize()
        row = {"set": name}
        for mode, kw in modes.items():
            row[mode] = stats(timed(torch, lambda s: ctx.overlap_boxes_device(boxes, stream=s, **kw), stream, a.repeats, a.warmup))
        row["closest_point"] = stats(timed(torch, lambda s: ctx.closest_point_device(pts, stream=s), stream, a.repeats, a.warmup))
        m = min(a.count_boxes, a.boxes)
        cnt, _, st = ctx.overlap_boxes(b_np[:m], counting=True)
        row["node_visits_per_box"] = st.node_visits / m
        row["tri_tests_per_box"] = st.tri_tests / m
        row["candidates_per_box"] = float(cnt.mean())
        row["occupied"] = float((cnt > 0).mean())
        res["sets"].append(row)
        print(json.dumps(row), flush=True)
        del boxes, pts
    if a.grid > 0:
        grid = voxel_grid(torch, lo, hi, a.grid)
        torch.cuda.synchronize()
        row = {"grid": a.grid, "voxels": a.grid ** 3}
        for mode in ("count", "any"):
            row[mode] = stats(timed(torch, lambda s: ctx.overlap_boxes_device(grid, stream=s, **modes[mode]), stream, max(3, a.repeats // 2), 1))
        occ = ctx.overlap_boxes_device(grid, max_ids=0, any=True)
        torch.cuda.synchronize()
        row["occupied"] = float(occ.count.to(torch.float64).mean().item())
        res["voxel_grid"] = row
        print(json.dumps(row), flush=True)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
