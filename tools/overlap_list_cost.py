"""What the overlap lists (rt_overlap_*_device_list) cost beside the capped calls on the same records, written to one JSON file.

  voxel grid    --grid^3 (default 128) voxels over the box of --teapots (default 8) teapots on a grid: most voxels touch nothing.
                list (capacity = the total, known from a first call), offsets only (capacity 0), the capped call count-only
                (max_ids 0) and with max_ids 16.  bytes: what the list call writes (offsets and ids) against n x 16 x 8 + n x 4.
  surface boxes --surface-boxes (default 262 144) boxes of 4 % to 12 % of a teapot's extent centred on surface samples of the same
                scene: rows of tens to hundreds of entries, the lengths an insertion threshold decides about.
  bodies        the scene of tools/scene_triangles_cost.py (--bodies spheres of 1 280 triangles, neighbours interpenetrate), one
                reference per triangle with against = -1: the same four calls by reference.
  sort rows     a strip of triangles and --sort-copies (default 256) copies of one box that touches exactly L of them, for L = 17, the
                LDS tile and --long-row (default 50 000): the list call and the offsets-only call; their difference is the second walk
                and the sort.  Under a kernel trace the k_list_sort launches appear in this order, --warmup + --repeats times each.
  device_ms     HIP events around the call on a torch stream: the median of --repeats calls after --warmup calls, the calls of a row
                taking turns.

  --variant     librt_mi355x_<variant>.so (make exp EXP_NAME=<variant> EXP_FLAGS="-DRT_LIST_INSERT_MAX=.. -DRT_LIST_LDS_TILE=.."), with
                --insert-max / --tile naming what it was built with

python3 tools/overlap_list_cost.py --out overlap_list_cost_results.json"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.closest_point_cost import stats  # noqa: E402
from tools.scene_triangles_cost import alternated, bodies, icosphere  # noqa: E402
from vulkan_raytracing_amd import RtContext, api, host  # noqa: E402

RES = os.path.join(ROOT, "resources")


def thresholds():
    src = open(os.path.join(ROOT, "vulkan_raytracing_amd", "csrc", "rt_kernels.h")).read()
    return tuple(int(re.findall(r"^#define %s (\d+)" % n, src, re.M)[0]) for n in ("RT_LIST_INSERT_MAX", "RT_LIST_LDS_TILE"))


THRESHOLDS = None


def four_calls(torch, ctx, kind, records, stream, repeats, warmup):
    """the list call at capacity = total, the offsets-only call, the capped call count-only and with max_ids 16"""
    lst, cap = getattr(ctx, "overlap_%s_device_list" % kind), getattr(ctx, "overlap_%s_device" % kind)
    n = records.shape[0]
    total = int(lst(records, capacity=0).total)
    offsets = torch.empty(n + 1, dtype=torch.int64, device="cuda:0")
    ids = torch.empty((max(total, 1), 2), dtype=torch.int32, device="cuda:0")
    rows = (torch.empty((n, 16, 2), dtype=torch.int32, device="cuda:0"), torch.empty(n, dtype=torch.int32, device="cuda:0"))
    ms = alternated(torch, [lambda s: lst(records, stream=s, out=(offsets, ids)), lambda s: lst(records, stream=s, out=(offsets, None)),
                            lambda s: cap(records, max_ids=0, stream=s, out=(None, rows[1])), lambda s: cap(records, max_ids=16, stream=s, out=rows)],
                    stream, repeats, warmup)
    torch.cuda.synchronize()
    lengths = (offsets[1:] - offsets[:-1])
    ins = THRESHOLDS[0]
    q = torch.quantile(lengths.double(), torch.tensor([0.5, 0.9, 0.99], dtype=torch.float64, device="cuda:0")).tolist() if n <= (1 << 24) else []
    row = {"row_length_p50_p90_p99": q, "records": n, "total_pairs": total, "empty_rows": float((lengths == 0).double().mean().item()), "longest_row": int(lengths.max().item()),
           "rows_sorted_by_k_list_sort": int((lengths > ins).sum().item()),
           "list": stats(ms[0]), "offsets_only": stats(ms[1]), "capped_count": stats(ms[2]), "capped_ids16": stats(ms[3]),
           "list_bytes_written": (n + 1) * 8 + total * 8, "capped_ids16_bytes_written": n * 16 * 8 + n * 4}
    row["list_over_capped_count"] = row["list"]["median_ms"] / row["capped_count"]["median_ms"]
    row["list_over_capped_ids16"] = row["list"]["median_ms"] / row["capped_ids16"]["median_ms"]
    return row


def teapots(n):
    g = host.SceneGeometry([os.path.join(RES, "teapot.obj")])
    side = int(np.ceil(n ** (1 / 3)))
    p = np.asarray(g.verts, np.float32).reshape(-1, 6)[:, :3]
    step = float((p.max(0) - p.min(0)).max()) * 1.25
    inst = [host.make_instance(np.array([1, 0, 0, step * (i % side), 0, 1, 0, step * ((i // side) % side), 0, 0, 1, step * (i // (side * side))], np.float32), i, 0)
            for i in range(n)]
    inst = np.array(inst, api.INSTANCE_DTYPE)
    for r in inst:
        r["custom_index_and_mask"] = (int(r["custom_index_and_mask"]) & 0xFFFFFF) | (0xFF << 24)
    lo = p.min(0).astype(np.float64)
    hi = p.max(0).astype(np.float64) + step * (side - 1)
    return g, inst, lo, hi


def strip(n_tris):
    k = np.arange(n_tris, dtype=np.float32)
    z = 0 * k
    pos = np.stack([np.stack([k, z, z], 1), np.stack([k + 1, z, z], 1), np.stack([k, z + 1, z], 1)], axis=1).reshape(-1, 3)
    verts = np.concatenate([pos, np.tile([[0, 0, 1]], (len(pos), 1))], axis=1).astype(np.float32).reshape(-1)
    inst = np.array([host.make_instance(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), 0, 0)], api.INSTANCE_DTYPE)
    inst[0]["custom_index_and_mask"] = 0xFF << 24
    return verts, np.arange(len(pos), dtype=np.uint32), [(0, 0, n_tris)], inst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="overlap_list_cost_results.json")
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--teapots", type=int, default=8)
    ap.add_argument("--surface-boxes", type=int, default=1 << 18)
    ap.add_argument("--variant", default=None)
    ap.add_argument("--insert-max", type=int, default=0)
    ap.add_argument("--tile", type=int, default=0)
    ap.add_argument("--bodies", type=int, default=512)
    ap.add_argument("--subdiv", type=int, default=3)
    ap.add_argument("--long-row", type=int, default=50000)
    ap.add_argument("--sort-copies", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from tools.overlap_cost import voxel_grid
    stream = torch.cuda.Stream()
    global THRESHOLDS
    ins, tile = thresholds()
    ins, tile = a.insert_max or ins, a.tile or tile
    THRESHOLDS = (ins, tile)
    res = {"RT_LIST_INSERT_MAX": ins, "RT_LIST_LDS_TILE": tile, "variant": a.variant}
    ctx = RtContext(0, variant=a.variant)
    res["device"] = ctx.device_info
    if a.grid > 0 or a.surface_boxes > 0:
        g, inst, lo, hi = teapots(a.teapots)
        ctx.upload_geometry(g.verts, g.idx, g.ranges)
        ctx.set_instances(inst)
    if a.surface_boxes > 0:
        rng = np.random.default_rng(3)
        p = np.asarray(g.verts, np.float32).reshape(-1, 6)[:, :3].astype(np.float64)
        ext = float((p.max(0) - p.min(0)).max())
        k = rng.integers(0, len(p), a.surface_boxes)
        c = p[k] + inst["transform"][rng.integers(0, len(inst), a.surface_boxes)][:, [3, 7, 11]].astype(np.float64)
        h = 0.5 * ext * rng.uniform(0.04, 0.12, (a.surface_boxes, 1))
        b = np.zeros((a.surface_boxes, 8), np.float32)
        b[:, 0:3] = c - h; b[:, 4:7] = c + h
        boxes = torch.from_numpy(b).to("cuda:0")
        torch.cuda.synchronize()
        row = four_calls(torch, ctx, "boxes", boxes, stream, a.repeats, a.warmup)
        row.update(surface_boxes=a.surface_boxes, teapots=a.teapots)
        res["surface_boxes"] = row
        print(json.dumps(row), flush=True)
        del boxes
    if a.grid > 0:
        grid = voxel_grid(torch, lo, hi, a.grid)
        torch.cuda.synchronize()
        row = four_calls(torch, ctx, "boxes", grid, stream, a.repeats, a.warmup)
        row.update(grid=a.grid, teapots=a.teapots)
        res["voxel_grid"] = row
        print(json.dumps(row), flush=True)
        del grid
    if a.bodies > 0:
        pos, faces = icosphere(a.subdiv)
        inst = bodies(a.bodies)
        for r in inst:
            r["custom_index_and_mask"] = (int(r["custom_index_and_mask"]) & 0xFFFFFF) | (0xFF << 24)
        ctx.upload_geometry(np.concatenate([pos, pos], axis=1).astype(np.float32).reshape(-1), faces.astype(np.uint32).reshape(-1), [(0, 0, len(faces))])
        ctx.set_instances(inst)
        nf = len(faces)
        refs = torch.from_numpy(api.triangle_refs(np.repeat(np.arange(a.bodies), nf), np.tile(np.arange(nf), a.bodies))).to("cuda:0")
        torch.cuda.synchronize()
        row = four_calls(torch, ctx, "scene_triangles", refs, stream, a.repeats, a.warmup)
        row.update(bodies=a.bodies, triangles_per_body=nf)
        res["bodies"] = row
        print(json.dumps(row), flush=True)
        del refs
    if a.sort_copies > 0:
        lens = [ins + 1, tile, a.long_row]
        verts, idx, ranges, inst = strip(max(lens) + 8)
        ctx.upload_geometry(verts, idx, ranges)
        ctx.set_instances(inst)
        res["sort_rows"] = []
        for L in lens:
            b = np.zeros((a.sort_copies, 8), np.float32)
            b[:, 0:3] = [-0.5, 0.125, -0.5]; b[:, 4:7] = [L - 0.5, 0.25, 0.5]
            boxes = torch.from_numpy(b).to("cuda:0")
            total = int(ctx.overlap_boxes_device_list(boxes, capacity=0).total)
            assert total == L * a.sort_copies, (total, L)
            offsets = torch.empty(a.sort_copies + 1, dtype=torch.int64, device="cuda:0")
            ids = torch.empty((total, 2), dtype=torch.int32, device="cuda:0")
            ms = alternated(torch, [lambda s: ctx.overlap_boxes_device_list(boxes, stream=s, out=(offsets, ids)),
                                    lambda s: ctx.overlap_boxes_device_list(boxes, stream=s, out=(offsets, None))], stream, a.repeats, a.warmup)
            torch.cuda.synchronize()
            want = torch.arange(L, dtype=torch.int32, device="cuda:0")
            assert torch.equal(ids.view(a.sort_copies, L, 2)[:, :, 1], want[None].expand(a.sort_copies, L)), L
            row = {"row_length": L, "rows": a.sort_copies, "list": stats(ms[0]), "offsets_only": stats(ms[1]),
                   "second_walk_and_sort_ms": float(np.median(ms[0]) - np.median(ms[1]))}
            res["sort_rows"].append(row)
            print(json.dumps(row), flush=True)
    ctx.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
