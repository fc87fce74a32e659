"""What the broad phase over the scene's instances costs, written to one JSON file.

  scene         N small bodies (octahedra of radius 0.3, random rotations) on a jittered grid of spacing 1, the TLAS built on the device
                (rt_set_instances_device); N = 4 096 and 65 536.  With a margin of 0.2 a body lists about ten others.
  (a) dense     rt_instance_pairs_device (every body against the others, the margin above, a persistent pair buffer) beside the dense
                comparison of the same canonical boxes in torch: the N x N closed test in blocks of --block rows, the pairs of a block
                extracted with nonzero.  Both produce the complete list; they are compared as sets.
  (b) contact   the broad phase at margin 0 and rt_overlap_instances_device(any=True) over the listed pairs (the total read on the host
                in between), beside the only device-side route without a broad phase: rt_overlap_instances_device(against=-1,
                any=True) for all N bodies.  Both say which bodies touch something; the answers are compared.
  device_ms     HIP events around the calls on a torch stream (for (b) around the whole sequence, the host read of the total
                included); the two sides of a comparison take turns: the median of --repeats calls of each after --warmup calls of
                each, with the spread (min .. max).

python3 tools/instance_broadphase_cost.py --out instance_broadphase_cost_results.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.instance_broadphase_reference import canonical_boxes  # noqa: E402
from tools.closest_point_cost import stats  # noqa: E402
from tools.triangle_overlap_cost import alternated  # noqa: E402
from vulkan_raytracing_amd import RtContext, api, host  # noqa: E402

MARGIN = 0.2


def octahedron():
    P = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    tris = []
    for sx in (0, 1):
        for sy in (2, 3):
            for sz in (4, 5):
                a, b, c = P[sx], P[sy], P[sz]
                tris.append([sx, sy, sz] if np.dot(np.cross(b - a, c - a), a + b + c) > 0 else [sx, sz, sy])
    return np.concatenate([P, P], axis=1).astype(np.float32).reshape(-1), np.array(tris, np.uint32).reshape(-1)


def bodies(dims, seed=7):
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    n = len(g)
    q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    t = g + rng.uniform(-0.2, 0.2, (n, 3))
    inst = np.zeros(n, api.INSTANCE_DTYPE)
    inst["transform"] = np.concatenate([0.3 * q, t[:, :, None]], axis=2).astype(np.float32).reshape(n, 12)
    inst["custom_index_and_mask"] = (np.arange(n, dtype=np.uint32) & 0xFFFFFF) | np.uint32(0xFF << 24)
    inst["mesh"] = 0
    return inst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="instance_broadphase_cost_results.json")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--block", type=int, default=1024)
    a = ap.parse_args()
    import torch
    verts, idx = octahedron()
    res = {"device": None, "margin": MARGIN, "sizes": {}}
    stream = torch.cuda.Stream()
    for dims in ((16, 16, 16), (64, 32, 32)):
        inst = bodies(dims)
        n = len(inst)
        ctx = RtContext(0)
        res["device"] = ctx.device_info
        ctx.upload_geometry(verts, idx, [(0, 0, 8)])
        d_inst = torch.from_numpy(inst.view(np.uint8).reshape(-1, 64).copy()).to("cuda:0")
        torch.cuda.synchronize()
        ctx.set_instances_device(d_inst)
        lo, hi = verts.reshape(-1, 6)[:, :3].min(0), verts.reshape(-1, 6)[:, :3].max(0)
        blo, bhi, has, _ = canonical_boxes(inst["transform"], np.tile(lo, (n, 1)), np.tile(hi, (n, 1)))
        assert has.all()
        t_lo, t_hi = torch.from_numpy(blo).to("cuda:0"), torch.from_numpy(bhi).to("cuda:0")
        near = torch.from_numpy(api.instance_refs(np.arange(n), -1, MARGIN)).to("cuda:0")
        contact = torch.from_numpy(api.instance_refs(np.arange(n), -1, 0.0)).to("cuda:0")
        offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda:0")
        pairs = torch.empty((32 * n, 4), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        seen = {}

        def broad(s):
            seen["broad"] = ctx.instance_pairs_device(near, out=(offsets, pairs), stream=s)

        def dense(s):
            m = torch.tensor(MARGIN, dtype=torch.float32, device="cuda:0")
            out = []
            with torch.cuda.stream(s):
                for b in range(0, n, a.block):
                    xlo, xhi = t_lo[b:b + a.block] - m, t_hi[b:b + a.block] + m
                    ok = (~(xlo[:, None, :] > t_hi[None]) & ~(xhi[:, None, :] < t_lo[None])).all(dim=2)
                    ij = ok.nonzero()
                    ij[:, 0] += b
                    out.append(ij[ij[:, 0] != ij[:, 1]])
                seen["dense"] = torch.cat(out)

        def routed(s):
            with torch.cuda.stream(s):
                _, _, total = ctx.instance_pairs_device(contact, out=(offsets, pairs), stream=s)
                t = int(total)
                touch = torch.zeros(n, dtype=torch.int64, device="cuda:0")
                if t:
                    hit, _ = ctx.overlap_instances_device(pairs[:t], any=True, stream=s)
                    touch.index_add_(0, pairs[:t, 0].long(), hit)
                seen["routed"], seen["routed_pairs"] = touch > 0, t

        def direct(s):
            seen["direct"] = ctx.overlap_instances_device(contact, any=True, stream=s)[0] > 0
        row = {"instances": n}
        b_ms, d_ms = alternated(torch, [broad, dense], stream, a.repeats, a.warmup)
        torch.cuda.synchronize()
        total = int(seen["broad"].total)
        got = seen["broad"].pairs[:total, :2].long()
        row["listed_pairs"] = total
        row["same_pairs"] = bool(total == len(seen["dense"]) and torch.equal(got, seen["dense"]))
        row["dense"] = {"instance_pairs": stats(b_ms), "torch_dense": stats(d_ms), "instance_pairs_over_dense": float(np.median(b_ms) / np.median(d_ms))}
        r_ms, o_ms = alternated(torch, [routed, direct], stream, a.repeats, a.warmup)
        torch.cuda.synchronize()
        row["contact_pairs_listed"] = seen["routed_pairs"]
        row["bodies_touching"] = int(seen["direct"].sum())
        row["same_answers"] = bool(torch.equal(seen["routed"], seen["direct"]))
        row["contact"] = {"broad_then_narrow": stats(r_ms), "against_everything": stats(o_ms), "broad_then_narrow_over_against_everything": float(np.median(r_ms) / np.median(o_ms))}
        _, _, st = ctx.instance_pairs(near.cpu().numpy(), capacity=total, counting=True)
        row["per_record"] = {"node_visits": st.node_visits / n, "box_tests": st.tri_tests / n, "tlas_nodes": n - 1}
        res["sizes"][str(n)] = row
        print(n, json.dumps(row), flush=True)
        ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
