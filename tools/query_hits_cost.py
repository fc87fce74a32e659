"""What all-hits queries (rt_intersect_device_hits) cost against the closest-hit query (rt_intersect_device_flags), on the cfg3 scene,
written to one JSON file.

  closest        rt_intersect_device_flags, flags 0, cull mask 0xFF: the yardstick
  k1, k4, k16    rt_intersect_device_hits with max_hits 1, 4, 16 and no counts (the walk prunes beyond the K-th entry)
  k4_counts      max_hits 4 with counts (the walk sees every candidate)
  count_only     max_hits 0 with counts

1 M and 8 M rays; camera-coherent primary rays and incoherent random rays (tools/query_cost.py's); HIP events around each query on a
torch stream, median of --repeats after --warmup.  Each row also has the mean number of candidates per ray.

python3 tools/query_hits_cost.py --out query_hits_cost_results.json"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.query_cost import primary_rays, random_rays  # noqa: E402
from tools.query_flags_cost import timed  # noqa: E402
from vulkan_raytracing_amd import RtContext, workloads  # noqa: E402

RES = os.path.join(ROOT, "resources")
SIZES = [1 << 20, 8 << 20]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="query_hits_cost_results.json")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mesh", default="standin")
    a = ap.parse_args()
    import torch
    wl = workloads.make("cfg3", RES, mesh=a.mesh)
    ctx = RtContext(0)
    wl.apply(ctx)
    stream = torch.cuda.Stream()
    res = {"workload": "cfg3", "mesh": wl.mesh_label, "device": ctx.device_info, "rows": []}
    for n in SIZES:
        for kind in ("primary", "random"):
            rays = torch.from_numpy(primary_rays(wl.uniforms, n) if kind == "primary" else random_rays(n)).to("cuda:0")
            torch.cuda.synchronize()
            row = {"rays": n, "kind": kind}
            row["closest"] = timed(torch, stream, lambda: ctx.intersect_device_flags(rays, stream=stream), a.repeats, a.warmup)
            for name, k, counts in (("k1", 1, False), ("k4", 4, False), ("k16", 16, False), ("k4_counts", 4, True), ("count_only", 0, True)):
                row[name] = timed(torch, stream, lambda: ctx.intersect_device_hits(rays, k, counts=counts, stream=stream), a.repeats, a.warmup)
                row[name + "_over_closest"] = row[name]["median_ms"] / row["closest"]["median_ms"]
            with torch.cuda.stream(stream):
                c = ctx.intersect_device_hits(rays, 0, stream=stream).count
            stream.synchronize()
            row["mean_candidates"] = float(c.double().mean().item())
            row["rays_with_candidates"] = float((c > 0).double().mean().item())
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            del rays, c
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
