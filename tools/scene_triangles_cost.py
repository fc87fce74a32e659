"""What asking about the scene's own triangles by reference costs, written to one JSON file.

  scene         --bodies spheres (default 512) of --subdiv subdivisions (default 3: 1 280 triangles each) on a jittered grid whose
                spacing lets neighbours interpenetrate; one reference per triangle of every body.
  by reference  rt_overlap_scene_triangles_device (against = -1) beside rt_overlap_triangles_device over the same world triangles
                expanded beforehand (rt_scene_triangles_device), whose kernel is the one the library had before the by-reference calls,
                and the expansion alone.  The plain call has no exclusion: it also tests every triangle against its own body.
  pair form     the triangles of body a against its nearest neighbour b only (against = b) beside the same references against every
                other body (against = -1).
  device_ms     HIP events around the call on a torch stream; the calls of a comparison take turns: the median of --repeats calls of
                each after --warmup calls of each, with the spread (min .. max).
  per query     node_visits and tri_tests of the host forms with counting, on the first --count-queries references.

python3 tools/scene_triangles_cost.py --out scene_triangles_cost_results.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.closest_point_cost import stats  # noqa: E402
from tools.triangle_overlap_cost import alternated  # noqa: E402
from vulkan_raytracing_amd import RtContext, api, host  # noqa: E402


def icosphere(subdiv):
    """(positions (nv, 3), faces (nf, 3)) of a unit sphere: an icosahedron subdivided `subdiv` times"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        mid, g = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return np.array(v), np.array(f, np.int64)


def bodies(n, seed=1):
    """n instance records of mesh 0 on a jittered cubic grid, radius 0.6 at spacing 1: neighbours interpenetrate; random rotations"""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n ** (1 / 3)))
    out = []
    for i in range(n):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        c = np.array([i % side, (i // side) % side, i // (side * side)], np.float64) + rng.uniform(-0.1, 0.1, 3)
        M = np.concatenate([0.6 * q, c[:, None]], axis=1).astype(np.float32).reshape(12)
        out.append(host.make_instance(M, i, 0))
    return np.array(out, api.INSTANCE_DTYPE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="scene_triangles_cost_results.json")
    ap.add_argument("--bodies", type=int, default=512)
    ap.add_argument("--subdiv", type=int, default=3)
    ap.add_argument("--count-queries", type=int, default=1 << 17)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    pos, faces = icosphere(a.subdiv)
    verts = np.concatenate([pos, pos], axis=1).astype(np.float32).reshape(-1)
    idx = faces.astype(np.uint32).reshape(-1)
    inst = bodies(a.bodies)
    for r in inst:
        r["custom_index_and_mask"] = (int(r["custom_index_and_mask"]) & 0xFFFFFF) | (0xFF << 24)
    ctx = RtContext(0)
    ctx.upload_geometry(verts, idx, [(0, 0, len(faces))])
    ctx.set_instances(inst)
    nf = len(faces)
    body, prim = np.repeat(np.arange(a.bodies), nf), np.tile(np.arange(nf), a.bodies)
    centres = inst["transform"][:, [3, 7, 11]].astype(np.float64)
    d = np.linalg.norm(centres[:, None] - centres[None], axis=2) + np.eye(a.bodies) * 1e9
    neighbour = d.argmin(axis=1)
    others_np, pair_np = api.triangle_refs(body, prim), api.triangle_refs(body, prim, against=neighbour[body])
    others, pair = torch.from_numpy(others_np).to("cuda:0"), torch.from_numpy(pair_np).to("cuda:0")
    stream = torch.cuda.Stream()
    world = ctx.scene_triangles_device(others)
    torch.cuda.synchronize()
    n = len(others_np)
    res = {"device": ctx.device_info, "bodies": a.bodies, "triangles_per_body": nf, "references": n, "rows": []}
    modes = {"count": dict(max_ids=0), "ids16": dict(max_ids=16), "any": dict(max_ids=0, any=True)}
    for mode, kw in modes.items():
        r_ms, p_ms, e_ms, q_ms = alternated(torch, [lambda s: ctx.overlap_scene_triangles_device(others, stream=s, **kw),
                                                    lambda s: ctx.overlap_triangles_device(world, stream=s, **kw),
                                                    lambda s: ctx.scene_triangles_device(others, stream=s, out=world),
                                                    lambda s: ctx.overlap_scene_triangles_device(pair, stream=s, **kw)], stream, a.repeats, a.warmup)
        row = {"mode": mode, "by_reference": stats(r_ms), "plain_on_expanded": stats(p_ms), "expansion": stats(e_ms), "pair_form": stats(q_ms),
               "by_reference_over_plain_plus_expansion": float(np.median(r_ms) / (np.median(p_ms) + np.median(e_ms))),
               "pair_form_over_by_reference": float(np.median(q_ms) / np.median(r_ms))}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    m = min(a.count_queries, n)
    world_np = world.cpu().numpy()
    per = {}
    for name, call in (("by_reference", lambda: ctx.overlap_scene_triangles(others_np[:m], counting=True)), ("pair_form", lambda: ctx.overlap_scene_triangles(pair_np[:m], counting=True)),
                       ("plain_on_expanded", lambda: ctx.overlap_triangles(world_np[:m], counting=True))):
        cnt, _, st = call()
        per[name] = {"node_visits": st.node_visits / m, "tri_tests": st.tri_tests / m, "candidates": float(cnt.mean()), "hit_share": float((cnt > 0).mean())}
    res["per_query"] = per
    print(json.dumps(per), flush=True)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
