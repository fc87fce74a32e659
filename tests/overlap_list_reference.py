"""The reference for rt_overlap_boxes_device_list, rt_overlap_triangles_device_list and rt_overlap_scene_triangles_device_list
(include/rt_api.h "Overlap lists"; DESIGN.md §5 "Overlap lists"), without a tree: the candidate sets are those of the capped calls, so
the pairs come from overlap_reference, triangle_overlap_reference and scene_triangle_reference as they are; what is new here is their
CSR form and the rule of which rows a capacity lets through.

 * csr: offsets (n + 1,) uint64 and ids (T, 2) int32 of kept pairs, every row in ascending (inst, prim) order;
 * boxes_csr, triangles_csr, refs_csr: csr of the three references' pairs;
 * written, expected_ids: the written-rows rule restated in numpy: row i is written if and only if offsets[i + 1] <= capacity, and no
   other byte of the ids buffer changes;
 * strip_scene, strip_boxes: a strip of lattice triangles and boxes that touch exactly m of them, for rows of chosen lengths;
 * thresholds: RT_LIST_INSERT_MAX and RT_LIST_LDS_TILE as csrc/rt_kernels.h defines them."""
import os
import re

import numpy as np

from tests import overlap_reference as orf
from tests import scene_triangle_reference as stf
from tests import triangle_overlap_reference as trf
from vulkan_raytracing_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x7F   # the byte a test fills its ids buffer with before a call


def thresholds():
    """(RT_LIST_INSERT_MAX, RT_LIST_LDS_TILE) as csrc/rt_kernels.h defines them"""
    src = open(os.path.join(ROOT, "vulkan_raytracing_amd", "csrc", "rt_kernels.h")).read()
    out = []
    for name in ("RT_LIST_INSERT_MAX", "RT_LIST_LDS_TILE"):
        m = re.findall(r"^#define %s (\d+)" % name, src, re.M)
        assert len(m) == 1, name
        out.append(int(m[0]))
    return tuple(out)


def csr(scene, n, bi, ti, keep):
    """offsets (n + 1,) uint64 and ids (T, 2) int32 of the kept pairs (record bi[k], triangle ti[k]): row i is every kept triangle of
    record i, ascending by (inst, prim) (closest_reference.Scene orders its triangles so)"""
    bi, ti = np.asarray(bi)[keep], np.asarray(ti)[keep]
    order = np.lexsort((ti, bi))
    bi, ti = bi[order], ti[order]
    offsets = np.zeros(n + 1, np.uint64)
    offsets[1:] = np.cumsum(np.bincount(bi, minlength=n).astype(np.uint64), dtype=np.uint64)
    ids = np.stack([scene.inst[ti], scene.prim[ti]], axis=1).astype(np.int32).reshape(-1, 2)
    return offsets, ids


def boxes_csr(scene, boxes, cull_mask=0xFF, tris=None):
    tris = tris or orf.Triangles(scene)
    n = len(np.asarray(boxes, np.float32).reshape(-1, 8))
    bi, ti = orf.surviving_pairs(tris, boxes, cull_mask)
    return csr(scene, n, bi, ti, orf.candidates32(tris, boxes, bi, ti))


def triangles_csr(scene, q, cull_mask=0xFF, tris=None):
    tris = tris or trf.Triangles(scene)
    n = len(np.asarray(q, np.float32).reshape(-1, 12))
    qi, ti = trf.surviving_pairs(tris, q, cull_mask)
    return csr(scene, n, qi, ti, trf.candidates32(tris, q, qi, ti))


def from_rows(counts, rows):
    """the CSR form of (counts, rows) of a capped reference whose max_ids is no less than the largest count"""
    counts = np.asarray(counts).astype(np.int64)
    assert rows.shape[1] >= (counts.max() if len(counts) else 0)
    offsets = np.zeros(len(counts) + 1, np.uint64)
    offsets[1:] = np.cumsum(counts).astype(np.uint64)
    take = np.arange(rows.shape[1])[None, :] < counts[:, None]
    return offsets, np.ascontiguousarray(rows[take]).reshape(-1, 2).astype(np.int32)


def refs_csr(src, refs, cull_mask=0xFF):
    """scene_triangle_reference.overlaps with max_ids set to the largest count, in CSR form"""
    counts, _ = stf.overlaps(src, refs, cull_mask, max_ids=0)
    k = max(1, int(counts.max()) if len(counts) else 1)
    counts, rows = stf.overlaps(src, refs, cull_mask, max_ids=k)
    return from_rows(counts, rows)


def prefix_rows(offsets, ids, max_ids=16):
    """(counts uint32 (n,), rows int32 (n, max_ids, 2)): what the capped call with max_ids returns for these lists"""
    off = np.asarray(offsets).astype(np.int64)
    counts = np.diff(off)
    rows = np.full((len(counts), max_ids, 2), -1, np.int32)
    j = np.arange(max_ids)[None, :]
    take = j < counts[:, None]
    rows[take] = ids[(off[:-1, None] + j)[take]]
    return counts.astype(np.uint32), rows


def written(offsets, capacity):
    """(n,) bool: the rows a call with `capacity` records of ids writes: offsets[i + 1] <= capacity (an empty row has nothing to write
    either way)"""
    return np.asarray(offsets)[1:].astype(np.uint64) <= np.uint64(capacity)


def expected_ids(offsets, ids, capacity, fill=FILL):
    """the bytes of an ids buffer of `capacity` records that held `fill` in every byte before the call: the written rows in place,
    everything else as it was"""
    out = np.full(capacity * 8, fill, np.uint8)
    off = np.asarray(offsets).astype(np.int64)
    w = written(offsets, capacity)
    flat = np.ascontiguousarray(ids, np.int32).reshape(-1, 2).view(np.uint8).reshape(-1, 8)
    for i in np.nonzero(w & (np.diff(off) > 0))[0]:
        out[off[i] * 8:off[i + 1] * 8] = flat[off[i]:off[i + 1]].reshape(-1)
    return out


# ---- rows of chosen lengths

def strip_scene(n_tris, seed=211):
    """n_tris lattice triangles (k, 0, 0), (k + 1, 0, 0), (k, 1, 0) in a row, stored in a shuffled order so that neither a tree's leaves
    nor its walk meet them by ascending prim; instance 0 the identity, instance 1 the strip again eight units up"""
    rng = np.random.default_rng(seed)
    k = rng.permutation(n_tris).astype(np.float32)
    pos = np.stack([np.stack([k, 0 * k, 0 * k], 1), np.stack([k + 1, 0 * k, 0 * k], 1), np.stack([k, 0 * k + 1, 0 * k], 1)], axis=1).reshape(-1, 3)
    verts = np.concatenate([pos, np.tile([[0, 0, 1]], (len(pos), 1))], axis=1).astype(np.float32).reshape(-1)
    idx = np.arange(len(pos), dtype=np.uint32)
    inst = np.zeros(2, api.INSTANCE_DTYPE)
    for i, z in enumerate((0.0, 8.0)):
        inst[i]["transform"] = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, z], np.float32)
        inst[i]["custom_index_and_mask"] = i | (0xFF << 24)
        inst[i]["mesh"] = 0
    return verts, idx, [(0, 0, n_tris)], inst


def strip_box(m, both=False):
    """a box that touches exactly the triangles at positions 0 .. m - 1 of instance 0 (both: of both instances, 2 m of them)"""
    lo = np.array([-0.5, 0.125, -0.5], np.float32)
    hi = np.array([m - 0.5 if m else -0.25, 0.25, 8.5 if both else 0.5], np.float32)
    b = np.zeros(8, np.float32)
    b[0:3] = lo; b[4:7] = hi
    return b
