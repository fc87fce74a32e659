"""What the K nearest triangles of a point (rt_closest_point_device_hits) cost on the cfg3 scene (teapot + stand-in), beside the single
nearest one (rt_closest_point_device) on the same points, written to one JSON file.

  point sets    (a) surface samples displaced by up to 1 % of the scene diagonal; (b) points uniform in twice the scene box; both with
                r_max = inf, and with r_max = 1 % of the diagonal for the cases that count.  --points each (default 1 M).
  cases         K = 1, 4 and 16 without counts (the pruned walk, r_max = inf); K = 4 with counts and count only at the finite radius
                (with counts the walk is bounded by the radius alone).
  device_ms     HIP events around the call on a torch stream.  Every case is ALTERNATED call by call with rt_closest_point_device on
                the same records: the median of --repeats calls of each after --warmup calls, with the smallest and largest beside it
                (the run-to-run spread), and the ratio of the medians.
  per point     node_visits and tri_tests of the host form with counting (rt_closest_point_hits), on the first --count-points records.
  the check     K = 1 without counts prunes exactly as rt_closest_point does: both counters of the two calls must be EQUAL (exit status
                1 otherwise).  Nothing else here is a pass condition.

python3 tools/closest_hits_cost.py --out closest_hits_cost_results.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.closest_point_cost import point_sets, stats, world_triangles  # noqa: E402
from vulkan_raytracing_amd import RtContext, workloads  # noqa: E402

RES = os.path.join(ROOT, "resources")
#        name, K, counts, finite radius
CASES = (("K1", 1, False, False), ("K4", 4, False, False), ("K16", 16, False, False), ("K4_counts_r", 4, True, True), ("count_only_r", 0, True, True))


def alternated(torch, calls, stream, repeats, warmup):
    """the calls in turn, repeats + warmup rounds: one list of device times per call"""
    out = [[] for _ in calls]
    for i in range(warmup + repeats):
        for k, call in enumerate(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record(stream)
                call(stream)
                e1.record(stream)
            e1.synchronize()
            if i >= warmup:
                out[k].append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="closest_hits_cost_results.json")
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
    res = {"workload": "cfg3", "mesh": wl.mesh_label, "device": ctx.device_info, "triangles": int(len(tris[0])), "points": a.points, "diagonal": diag, "rows": []}
    m = min(a.count_points, a.points)
    equal = True
    for name in ("a", "b"):
        for case, K, counts, finite in CASES:
            pts_np = sets[name].copy()
            if finite:
                pts_np[:, 3] = np.float32(0.01 * diag)
            pts = torch.from_numpy(pts_np).to("cuda:0")
            out = (torch.empty((a.points, K, 5), dtype=torch.int32, device="cuda:0") if K else None, None,
                   torch.empty((a.points,), dtype=torch.int32, device="cuda:0") if counts else None)
            single = (torch.empty((a.points, 5), dtype=torch.int32, device="cuda:0"), None)
            torch.cuda.synchronize()
            rows_ms, single_ms = alternated(torch, (lambda s: ctx.closest_point_device_hits(pts, K, counts=counts, stream=s, out=out),
                                                    lambda s: ctx.closest_point_device(pts, stream=s, out=single)), stream, a.repeats, a.warmup)
            row = {"set": name, "case": case, "max_hits": K, "counts": counts, "r_max": float(pts_np[0, 3]),
                   "closest_point_hits": stats(rows_ms), "closest_point": stats(single_ms)}
            row["ratio_of_medians"] = row["closest_point_hits"]["median_ms"] / row["closest_point"]["median_ms"]
            h, c, st = ctx.closest_point_hits(pts_np[:m], K, counts=counts, counting=True)
            row["node_visits_per_point"] = st.node_visits / m
            row["tri_tests_per_point"] = st.tri_tests / m
            if c is not None:
                row["mean_count"] = float(c.mean()); row["max_count"] = int(c.max())
            if case == "K1":
                h1, st1 = ctx.closest_point(pts_np[:m], counting=True)
                row["closest_point_node_visits_per_point"] = st1.node_visits / m
                row["closest_point_tri_tests_per_point"] = st1.tri_tests / m
                row["counters_equal"] = (st.node_visits, st.tri_tests) == (st1.node_visits, st1.tri_tests)
                row["records_equal"] = h[:, 0].tobytes() == h1.tobytes()
                equal = equal and row["counters_equal"] and row["records_equal"]
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            del pts, out, single
    ctx.close()
    res["k1_counters_equal_closest_point"] = equal
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
