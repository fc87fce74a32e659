"""The reference for rt_closest_instances_device and rt_overlap_instances_device (include/rt_api.h; DESIGN.md §5 "Instance pairs"), without a
tree, built from scene_triangle_reference and triangle_distance_reference:

 * a record (inst, against, r_max) stands for the references (inst, p, against, r_max) of every triangle p of the source's mesh;
 * nearest: the canonical d2 of every (p, candidate) pair under the instance rule and the mask, the minimum by (d2, p) (the candidate of
   a p is already its minimum by (d2, inst, prim)), and then scene_triangle_reference.nearest for the reference of the winner: the
   answer is defined as that call's;
 * overlaps: the canonical predicate of every such pair: the summed counts and the first (p, inst, prim).

The pair values of a scene (every triangle as the query against every triangle as the candidate) are computed once and shared by every
record list, radius and mask; they are never written to."""
import numpy as np

from tests import closest_reference as cr
from tests import scene_triangle_reference as stf
from tests import triangle_distance_reference as tdr
from tests import triangle_overlap_reference as trf

F = np.float32


def records(inst, against=-1, r_max=np.inf):
    """(n, 4) int32 rows (inst, against, the bits of r_max, 0); api.instance_refs restated (the reference does not lean on the code under test)"""
    i, a, r = np.broadcast_arrays(*(np.asarray(x).reshape(-1) for x in (inst, against, r_max)))
    out = np.zeros((len(i), 4), np.int32)
    out[:, 0] = i; out[:, 1] = a
    out[:, 2] = np.ascontiguousarray(r, F).view(np.int32)
    return out


class Pairs:
    """a scene and, made on first use, the pair values of all its triangles"""

    def __init__(self, parts):
        self.parts = parts
        with np.errstate(all="ignore"):   # (void and non-invertible records)
            self.sc = cr.Scene(*parts)
            self.src = stf.Source(self.sc, *parts)
        self.n_inst = self.src.n_inst
        self.count, self.first = self.src.count, self.src.first
        self._d2 = None
        self._touch = {}

    def d2(self, chunk=1 << 18):
        """(T, T) float32: the canonical d2 of triangle row (as the query: its expanded record) against triangle column (as the candidate);
        NaN for an invalid query and where no feature has a value"""
        if self._d2 is None:
            sc = self.sc
            tr, ok, _ = stf.expand(self.src, stf.every_triangle(sc))
            out = np.full((sc.n_tris, sc.n_tris), np.nan, F)
            idx = np.nonzero(ok & tdr.valid_triangles(tr))[0]
            ta, tab, tac = (tuple(getattr(sc, name)[:, k][None, :] for k in range(3)) for name in ("a", "ab", "ac"))
            per = max(1, chunk // max(1, sc.n_tris))
            for k0 in range(0, len(idx), per):
                i = idx[k0:k0 + per]
                P = tuple(tuple(tr[i, 4 * v + k][:, None] for k in range(3)) for v in range(3))
                out[i] = tdr.tri_tri32(P, ta, tab, tac)[0]
            out.setflags(write=False)
            self._d2 = out
        return self._d2

    def touch(self, cull_mask):
        """(T, T) bool: the canonical predicate does not separate query row from candidate column, the candidate admitted by cull_mask"""
        if cull_mask not in self._touch:
            sc = self.sc
            q, _, _ = stf.expand(self.src, stf.every_triangle(sc))
            qi, ti = trf.surviving_pairs(self.src.tris, q, cull_mask)
            keep = trf.candidates32(self.src.tris, q, qi, ti)
            m = np.zeros((sc.n_tris, sc.n_tris), bool)
            m[qi[keep], ti[keep]] = True
            m.setflags(write=False)
            self._touch[cull_mask] = m
        return self._touch[cull_mask]

    def valid(self, irefs, distance):
        r = np.asarray(irefs, np.int32).reshape(-1, 4)
        ok = (r[:, 0] >= 0) & (r[:, 0] < self.n_inst) & (r[:, 1] >= -1) & (r[:, 1] < self.n_inst)
        if distance:
            with np.errstate(invalid="ignore"):
                ok &= r[:, 2].view(F) >= 0
        return ok

    def columns(self, inst, against, cull_mask):
        """(T,) bool: the candidates of a record: admitted, and of another instance (against < 0) or of that instance"""
        sc = self.sc
        return sc.admitted(cull_mask) & ((sc.inst != inst) if against < 0 else (sc.inst == against))

    def per_triangle_d2(self, iref, cull_mask=0xFF):
        """d2_p of every source triangle of one valid record (+inf bits aside: NaN where p has no candidate)"""
        inst, against = int(iref[0]), int(iref[1])
        r_max = np.asarray(iref[2:3], np.int32).view(F)[0]
        rows = slice(int(self.first[inst]), int(self.first[inst] + self.count[inst]))
        sub = self.d2()[rows][:, self.columns(inst, against, cull_mask)]
        with np.errstate(all="ignore"):
            ok = ~np.isnan(sub) & (sub <= r_max * r_max)
        if sub.shape[1] == 0:
            return np.full(sub.shape[0], np.nan, F)
        best = np.where(ok, sub, np.inf).min(axis=1).astype(F)
        return np.where(ok.any(axis=1), best, F(np.nan))

    def nearest(self, irefs, cull_mask=0xFF):
        """(HIT_DTYPE records, src_prims int32 (n,), (qu, qv) float32 (n, 2), the winners' references (n, 4))"""
        r = np.asarray(irefs, np.int32).reshape(-1, 4)
        src = np.full(len(r), -1, np.int32)
        ok = self.valid(r, True)
        for k in np.nonzero(ok)[0]:
            d2p = self.per_triangle_d2(r[k], cull_mask)
            has = np.nonzero(~np.isnan(d2p))[0]
            if len(has):
                src[k] = has[np.argmin(d2p[has])]   # (the first minimum: the smallest p)
        hit = src >= 0
        refs = np.zeros((len(r), 4), np.int32)
        refs[:, 0] = np.where(hit, r[:, 0], -1); refs[:, 1] = src; refs[:, 2] = np.where(hit, r[:, 1], -1); refs[:, 3] = r[:, 2]
        hits, quv = stf.nearest(self.src, refs, cull_mask)
        assert ((hits["inst"] >= 0) == hit).all()
        return hits, src, quv, refs

    def overlaps(self, irefs, cull_mask=0xFF):
        """(counts uint64 (n,), first4 int32 (n, 4): (p, inst, prim, 0) or (-1, -1, -1, 0))"""
        r = np.asarray(irefs, np.int32).reshape(-1, 4)
        counts = np.zeros(len(r), np.uint64)
        first4 = np.zeros((len(r), 4), np.int32)
        first4[:, :3] = -1
        m = self.touch(cull_mask)
        sc = self.sc
        for k in np.nonzero(self.valid(r, False))[0]:
            inst, against = int(r[k, 0]), int(r[k, 1])
            rows = slice(int(self.first[inst]), int(self.first[inst] + self.count[inst]))
            cols = np.nonzero(self.columns(inst, against, cull_mask))[0]
            sub = m[rows][:, cols]
            counts[k] = int(sub.sum())
            ps = np.nonzero(sub.any(axis=1))[0]
            if len(ps):
                c = cols[np.argmax(sub[ps[0]])]   # (columns are in (inst, prim) order)
                first4[k, :3] = (ps[0], sc.inst[c], sc.prim[c])
        return counts, first4


def every_triangle_of(pairs, irefs):
    """the (inst, p, against, r_max) references of every source triangle of every valid record, and the record of each"""
    r = np.asarray(irefs, np.int32).reshape(-1, 4)
    out, rec = [], []
    for k in np.nonzero(pairs.valid(r, False))[0]:
        n = int(pairs.count[r[k, 0]])
        out.append(stf.refs(r[k, 0], np.arange(n), r[k, 1], r[k, 2:3].view(F)[0]).reshape(-1, 4))
        rec.append(np.full(n, k, np.int64))
    if not out:
        return np.zeros((0, 4), np.int32), np.zeros(0, np.int64)
    return np.concatenate(out), np.concatenate(rec)
