"""What ray flags and cull masks (rt_intersect_device_flags) cost against the plain device query (rt_intersect_device), on the cfg3
scene, written to one JSON file.

  neutral        flags 0, cull mask 0xFF, no ray words, against rt_intersect_device closest hit (the claim: within a few per cent)
  cull_back      CULL_BACK_FACING on instances without FACING_CULL_DISABLE
  half_ring      a cull mask hiding half of a ring of 16 instances (masks alternate 1 and 2, cull mask 1)
  mixed          a 50/50 per-ray mix of closest and first hit in one call, against two separate rt_intersect_device calls

64 K, 1 M and 8 M rays; camera-coherent primary rays and incoherent random rays (tools/query_cost.py's); HIP events around each query on
a torch stream, median of --repeats after --warmup.

python3 tools/query_flags_cost.py --out query_flags_cost_results.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.query_cost import primary_rays, random_rays, stats  # noqa: E402
from vulkan_raytracing_amd import RtContext, api, workloads  # noqa: E402

RES = os.path.join(ROOT, "resources")
SIZES = [64 << 10, 1 << 20, 8 << 20]


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


def ring(inst, k=16, radius=6.0):
    """k copies of the scene's first instance on a ring about it, masks alternating 1 and 2"""
    base = inst[0]
    out = np.repeat(inst[:1], k)
    for i in range(k):
        t = base["transform"].copy().reshape(3, 4)
        a = 2 * np.pi * i / k
        t[0, 3] += radius * np.cos(a); t[2, 3] += radius * np.sin(a)
        out[i]["transform"] = t.reshape(12)
        out[i]["custom_index_and_mask"] = (int(base["custom_index_and_mask"]) & 0xFFFFFF) | ((1 if i % 2 == 0 else 2) << 24)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="query_flags_cost_results.json")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mesh", default="standin")
    a = ap.parse_args()
    import torch
    wl = workloads.make("cfg3", RES, mesh=a.mesh)
    ctx = RtContext(0)
    wl.apply(ctx)
    stream = torch.cuda.Stream()
    culling = wl.instances.copy()
    culling["sbt_offset_and_flags"] = 0   # no FACING_CULL_DISABLE
    res = {"workload": "cfg3", "mesh": wl.mesh_label, "device": ctx.device_info, "rows": []}
    for n in SIZES:
        for kind in ("primary", "random"):
            rays = torch.from_numpy(primary_rays(wl.uniforms, n) if kind == "primary" else random_rays(n)).to("cuda:0")
            words = torch.full((n,), -16777216, dtype=torch.int32, device="cuda:0")   # 0xFF000000
            words[torch.arange(n, device="cuda:0") % 2 == 1] |= api.RAY_FLAG_TERMINATE_ON_FIRST_HIT
            half = torch.arange(n, device="cuda:0") < n // 2
            torch.cuda.synchronize()
            row = {"rays": n, "kind": kind}
            ctx.set_instances(wl.instances)
            row["intersect_device"] = timed(torch, stream, lambda: ctx.intersect_device(rays, stream=stream), a.repeats, a.warmup)
            row["neutral"] = timed(torch, stream, lambda: ctx.intersect_device_flags(rays, stream=stream), a.repeats, a.warmup)
            row["neutral_over_plain"] = row["neutral"]["median_ms"] / row["intersect_device"]["median_ms"]
            row["mixed_one_call"] = timed(torch, stream, lambda: ctx.intersect_device_flags(rays, words=words, stream=stream), a.repeats, a.warmup)
            r0, r1 = rays[~half].contiguous(), rays[half].contiguous()
            row["mixed_two_calls"] = timed(torch, stream, lambda: (ctx.intersect_device(r0, stream=stream), ctx.intersect_device(r1, any_hit=True, stream=stream)),
                                           a.repeats, a.warmup)
            ctx.set_instances(culling)
            row["cull_back_plain"] = timed(torch, stream, lambda: ctx.intersect_device(rays, stream=stream), a.repeats, a.warmup)
            row["cull_back"] = timed(torch, stream, lambda: ctx.intersect_device_flags(rays, ray_flags=api.RAY_FLAG_CULL_BACK_FACING, stream=stream),
                                     a.repeats, a.warmup)
            ctx.set_instances(ring(wl.instances))
            row["ring16_plain"] = timed(torch, stream, lambda: ctx.intersect_device(rays, stream=stream), a.repeats, a.warmup)
            row["ring16_half_culled"] = timed(torch, stream, lambda: ctx.intersect_device_flags(rays, cull_mask=1, stream=stream), a.repeats, a.warmup)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            del rays, words
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
