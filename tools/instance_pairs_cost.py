"""What asking about a pair of bodies costs through the instance-pair calls, beside the composed way of answering the same question with
the per-triangle calls on the same tree, written to one JSON file.

  mesh          the largest mesh under resources/ (by triangles), loaded alone.
  shapes        `apart`: two instances of it one and a half diameters apart; `touching`: the same two interpenetrating; `one_vs_15`:
                one instance among fifteen others on a grid that lets neighbours interpenetrate.  Each shape is asked with --records
                records (default 64: the same pair, or the one body against the others, asked that often, so that the device is
                filled as a scene of many pairs fills it).
  distance      rt_closest_instances_device beside rt_closest_scene_triangle_device over every triangle's reference and a minimum of
                t per record on the device (torch).
  overlap       rt_overlap_instances_device beside rt_overlap_scene_triangles_device with max_ids = 0 and a sum per record.
  occupancy     the same with any=True beside the per-triangle call with any=True and a maximum per record.
  device_ms     HIP events around the call on a torch stream; the two calls of a comparison take turns: the median of --repeats calls
                of each after --warmup calls of each, with the spread (min .. max).
  per record    node_visits and tri_tests of the host forms with counting (those of a shared-bound walk depend on timing).

python3 tools/instance_pairs_cost.py --out instance_pairs_cost_results.json"""
import argparse
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.closest_point_cost import stats  # noqa: E402
from tools.triangle_overlap_cost import alternated  # noqa: E402
from vulkan_raytracing_amd import RtContext, api, host  # noqa: E402

RES = os.path.join(ROOT, "resources")


def largest_mesh():
    """(path, verts, idx, triangles) of the .obj under resources/ with the most triangles"""
    best = None
    for path in sorted(glob.glob(os.path.join(RES, "*.obj"))):
        try:
            g = host.SceneGeometry([path])
        except RuntimeError:
            continue
        n = sum(r[2] for r in g.ranges)
        if len(g.ranges) == 1 and (best is None or n > best[3]):
            best = (path, g.verts, g.idx, n)
    return best


def placed(centres, radius_scale=1.0, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for i, c in enumerate(centres):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        M = np.concatenate([radius_scale * q, np.asarray(c, np.float64)[:, None]], axis=1).astype(np.float32).reshape(12)
        r = host.make_instance(M, i, 0)
        r["custom_index_and_mask"] = (int(r["custom_index_and_mask"]) & 0xFFFFFF) | (0xFF << 24)
        out.append(r)
    return np.array(out, api.INSTANCE_DTYPE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="instance_pairs_cost_results.json")
    ap.add_argument("--records", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    path, verts, idx, nf = largest_mesh()
    pos = verts.reshape(-1, 6)[:, :3].astype(np.float64)
    centre, diam = (pos.min(0) + pos.max(0)) / 2, float(np.linalg.norm(pos.max(0) - pos.min(0)))
    grid = [np.array([i % 4, (i // 4) % 2, i // 8], np.float64) * 0.6 * diam for i in range(16)]
    shapes = {"apart": ([np.zeros(3), np.array([1.5 * diam, 0, 0])], 0, 1),
              "touching": ([np.zeros(3), np.array([0.25 * diam, 0.1 * diam, 0])], 0, 1),
              "one_vs_15": (grid, 5, -1)}
    res = {"device": None, "mesh": os.path.basename(path), "triangles": nf, "records": a.records, "shapes": {}}
    stream = torch.cuda.Stream()
    for name, (centres, src, against) in shapes.items():
        ctx = RtContext(0)
        res["device"] = ctx.device_info
        ctx.upload_geometry(verts, idx, [(0, 0, nf)])
        ctx.set_instances(placed([c - centre for c in centres]))
        n = a.records
        irefs_np = api.instance_refs(np.full(n, src), against)
        every_np = api.triangle_refs(np.full(n * nf, src), np.tile(np.arange(nf), n), against)
        irefs, every = torch.from_numpy(irefs_np).to("cuda:0"), torch.from_numpy(every_np).to("cuda:0")
        torch.cuda.synchronize()
        seen = {}

        def pair_distance(s):
            seen["pair_t"] = ctx.closest_instances_device(irefs, stream=s).t

        def composed_distance(s):
            with torch.cuda.stream(s):
                seen["composed_t"] = ctx.closest_scene_triangle_device(every, stream=s).t.view(n, nf).min(dim=1).values

        def pair_overlap(s, any=False):
            seen["pair_any" if any else "pair_count"] = ctx.overlap_instances_device(irefs, any=any, stream=s)[0]

        def composed_overlap(s, any=False):
            with torch.cuda.stream(s):
                c = ctx.overlap_scene_triangles_device(every, max_ids=0, any=any, stream=s).count.view(n, nf)
                seen["composed_any" if any else "composed_count"] = c.max(dim=1).values if any else c.sum(dim=1, dtype=torch.int64)
        row = {}
        for what, calls in (("distance", (pair_distance, composed_distance)), ("overlap", (pair_overlap, composed_overlap)),
                            ("occupancy", (lambda s: pair_overlap(s, True), lambda s: composed_overlap(s, True)))):
            p_ms, c_ms = alternated(torch, list(calls), stream, a.repeats, a.warmup)
            row[what] = {"instance_pairs": stats(p_ms), "composed": stats(c_ms), "instance_pairs_over_composed": float(np.median(p_ms) / np.median(c_ms))}
        torch.cuda.synchronize()
        row["same_answers"] = bool(torch.equal(seen["pair_t"], seen["composed_t"]) and torch.equal(seen["pair_count"], seen["composed_count"]) and
                                   torch.equal(seen["pair_any"], seen["composed_any"].to(torch.int64)))
        row["t"] = float(seen["pair_t"][0]); row["pairs"] = int(seen["pair_count"][0])
        per = {}
        _, _, st = ctx.closest_instances(irefs_np, counting=True)
        per["distance_instance_pairs"] = {"node_visits": st.node_visits / n, "tri_tests": st.tri_tests / n}
        _, st = ctx.closest_scene_triangle(every_np, counting=True)
        per["distance_composed"] = {"node_visits": st.node_visits / n, "tri_tests": st.tri_tests / n}
        for any in (False, True):
            _, _, st = ctx.overlap_instances(irefs_np, any=any, counting=True)
            per[("occupancy" if any else "overlap") + "_instance_pairs"] = {"node_visits": st.node_visits / n, "tri_tests": st.tri_tests / n}
            _, _, st = ctx.overlap_scene_triangles(every_np, max_ids=0, any=any, counting=True)
            per[("occupancy" if any else "overlap") + "_composed"] = {"node_visits": st.node_visits / n, "tri_tests": st.tri_tests / n}
        row["per_record"] = per
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
