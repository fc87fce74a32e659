"""The reference for rt_instance_pairs_device (include/rt_api.h; DESIGN.md §5 "Instance broad phase"), in numpy, without a tree and
straight from the definition:

 * the canonical box of instance i: the eight corners of the exact bounds [lo, hi] of its mesh's active triangles through o2w in
   binary64 (M_r0 p0 + M_r1 p1 + M_r2 p2 + M_r3 in that order), each rounded once to binary32, their bounds blo and bhi, widened by
   e = 2^-13 mw, mw = max_r (|M_r0| bm_0 + |M_r1| bm_1 + |M_r2| bm_2 + |M_r3|) in binary32, unfused, left to right, bm_k = max(|lo_k|, |hi_k|);
   no box when a row sum is not finite;
 * a valid source: inst and against in range, r_max >= 0, not void (tree_reference.padded_world_box and the rule of void_records), a
   mesh with an active triangle, a box;
 * the candidates of (i, against, m): a box, (mask & cull_mask) != 0 (a void record has mask 0), j != i with against == -1, j == against
   otherwise, j > i with `above`, and on every axis !(Box(i).lo - m > Box(j).hi) and !(Box(i).hi + m < Box(j).lo) in binary32;
 * the rows (inst, j, the bits of r_max, 0) in ascending j, in CSR form."""
import numpy as np

from tests.tree_reference import INST_BOX_LIMIT, active_bounds, padded_world_box

F = np.float32
OB_ABS = F(2.0 ** -13)


def mesh_bounds(verts6, idx, ranges):
    """(lo, hi) float32 (meshes, 3): the exact bounds of the vertices of every mesh's active triangles (none: 3e38, -3e38)"""
    verts = np.asarray(verts6, F).reshape(-1)
    idx = np.asarray(idx, np.int64)
    lo, hi = [], []
    for ff, fi, pc in ranges:
        ix = idx[fi:fi + 3 * pc].reshape(-1, 3)
        p = verts[ff:].reshape(-1, 6)[:, :3]
        a, b = active_bounds(p[ix]) if pc else (np.full(3, 3.0e38, F), np.full(3, -3.0e38, F))
        lo.append(a); hi.append(b)
    return np.array(lo, F).reshape(-1, 3), np.array(hi, F).reshape(-1, 3)


def canonical_boxes(o2w, lo, hi):
    """o2w (n, 12), lo and hi (n, 3) -> (box_lo, box_hi float32 (n, 3), has_box bool (n,), mw float32 (n,))"""
    M32 = np.asarray(o2w, F).reshape(-1, 3, 4)
    M = M32.astype(np.float64)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    corner = np.array([[(c >> a) & 1 for a in range(3)] for c in range(8)], bool)
    p = np.where(corner[None], hi.astype(np.float64)[:, None, :], lo.astype(np.float64)[:, None, :])   # (n, 8, 3)
    with np.errstate(all="ignore"):
        v = ((M[:, None, :, 0] * p[:, :, None, 0] + M[:, None, :, 1] * p[:, :, None, 1]) + M[:, None, :, 2] * p[:, :, None, 2]) + M[:, None, :, 3]
        v32 = v.astype(F)                                   # (n, 8 corners, 3 rows)
        blo = np.fmin(F(3.0e38), np.fmin.reduce(v32, axis=1))
        bhi = np.fmax(F(-3.0e38), np.fmax.reduce(v32, axis=1))
        bm = np.maximum(np.abs(lo), np.abs(hi))              # (n, 3)
        A = np.abs(M32)
        rows = ((A[:, :, 0] * bm[:, None, 0] + A[:, :, 1] * bm[:, None, 1]).astype(F) + A[:, :, 2] * bm[:, None, 2]).astype(F) + A[:, :, 3]
        rows = rows.astype(F)                               # (n, 3)
        finite = (rows <= F(3.4028234e38)).all(axis=1)
        mw = np.fmax(F(0), np.fmax.reduce(rows, axis=1)).astype(F)
        e = (OB_ABS * mw).astype(F)
        return (blo - e[:, None]).astype(F), (bhi + e[:, None]).astype(F), finite & ~(lo[:, 0] > hi[:, 0]), mw


class BroadPhase:
    """the canonical boxes of a scene's instances and the rows of any record list"""

    def __init__(self, parts):
        verts, idx, ranges, inst = parts
        self.parts = parts
        self.n_inst = len(inst)
        mesh = np.asarray(inst["mesh"], np.int64)
        self.o2w = np.asarray(inst["transform"], F).reshape(-1, 12)
        mlo, mhi = mesh_bounds(verts, idx, ranges)
        self.lo, self.hi = mlo[mesh], mhi[mesh]
        self.active = ~(self.lo[:, 0] > self.hi[:, 0])
        self.box_lo, self.box_hi, self.has_box, self.mw = canonical_boxes(self.o2w, self.lo, self.hi)
        plo, phi = padded_world_box(self.o2w, self.lo, self.hi)
        with np.errstate(invalid="ignore"):
            inside = (np.abs(plo) < INST_BOX_LIMIT).all(axis=1) & (np.abs(phi) < INST_BOX_LIMIT).all(axis=1)
        self.void = ~(np.isfinite(self.o2w).all(axis=1) & inside) | ~self.active
        self.mask = np.where(self.void, 0, np.asarray(inst["custom_index_and_mask"], np.int64) >> 24)
        self.source = self.has_box & ~self.void & self.active
        for a in (self.box_lo, self.box_hi, self.has_box, self.mask, self.source):
            a.setflags(write=False)

    def row(self, inst, against, m, cull_mask=0xFF, above=False):
        """the ascending candidates j of one record (int64 array)"""
        n = self.n_inst
        m = F(m)
        if not (0 <= inst < n and -1 <= against < n) or not m >= 0 or not self.source[inst]:
            return np.zeros(0, np.int64)
        with np.errstate(all="ignore"):
            xlo = (self.box_lo[inst] - m).astype(F)
            xhi = (self.box_hi[inst] + m).astype(F)
            ok = self.has_box & ((self.mask & cull_mask) != 0) & ~(xlo[None] > self.box_hi).any(axis=1) & ~(xhi[None] < self.box_lo).any(axis=1)
        j = np.arange(n)
        ok &= (j != inst) if against < 0 else (j == against)
        if above:
            ok &= j > inst
        return np.nonzero(ok)[0]

    def rows(self, irefs, cull_mask=0xFF, above=False):
        """(offsets uint64 (n + 1,), pairs int32 (T, 4)): row i holds (inst, j, the bits of r_max, 0) in ascending j"""
        r = np.asarray(irefs, np.int32).reshape(-1, 4)
        out, offsets = [], np.zeros(len(r) + 1, np.uint64)
        for k in range(len(r)):
            js = self.row(int(r[k, 0]), int(r[k, 1]), r[k, 2:3].view(F)[0], cull_mask, above)
            rec = np.zeros((len(js), 4), np.int32)
            rec[:, 0] = r[k, 0]; rec[:, 1] = js; rec[:, 2] = r[k, 2]
            out.append(rec)
            offsets[k + 1] = offsets[k] + np.uint64(len(js))
        return offsets, (np.concatenate(out) if out else np.zeros((0, 4), np.int32))


def written(offsets, pairs, capacity, fill):
    """what a call with `capacity` leaves in a (capacity, 4) buffer that held `fill`: the rows that end within the capacity"""
    out = np.array(fill, np.int32, copy=True).reshape(capacity, 4)
    for i in range(len(offsets) - 1):
        o0, o1 = int(offsets[i]), int(offsets[i + 1])
        if o1 <= capacity:
            out[o0:o1] = pairs[o0:o1]
    return out
