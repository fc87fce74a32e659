"""Two references for rt_overlap_boxes_device (include/rt_api.h; DESIGN.md §5 "Box overlaps"), neither with a tree:

 * brute32: the canonical binary32 predicate restated in numpy from the header and DESIGN text, over every (box, instance, triangle)
   pair.  numpy's float32 +, -, * are IEEE; the library's explicit fused operations (dot3, cross3, xform_point, xform_vec) go through
   tests/closest_reference.py's fma32, an exactly rounded binary32 fma; min / max are np.fmin / np.fmax (fminf / fmaxf).  The GPU is held
   to it bit for bit.
 * brute64: the same thirteen axes in binary64 on the same binary32 A, B, C, lo, hi, with the separation of every pair: the largest gap
   over the axes (negative: the smallest penetration), each relative to the magnitudes that enter its projection.

Step 2 of the predicate (the box axes on lo / hi) compares binary32 numbers and is exact in both, so both evaluate the remaining axes on
the pairs that survive it only."""
import numpy as np

from tests.closest_reference import F, cross3, dot3

ANY = 0x1


class Triangles:
    """the world triangles of a closest_reference.Scene as the predicate forms them: A = xform_point(o2w, v0), B = A + ab, C = A + ac in
    binary32 (Scene.a / ab / ac are the canonical transforms), their bounds, and which of them are finite"""

    def __init__(self, scene):
        self.scene = scene
        with np.errstate(all="ignore"):
            self.A = np.asarray(scene.a, F).reshape(-1, 3)
            self.B = (self.A + np.asarray(scene.ab, F).reshape(-1, 3)).astype(F)
            self.C = (self.A + np.asarray(scene.ac, F).reshape(-1, 3)).astype(F)
        self.finite = np.isfinite(self.A).all(-1) & np.isfinite(self.B).all(-1) & np.isfinite(self.C).all(-1)
        self.mn = np.fmin(np.fmin(self.A, self.B), self.C)
        self.mx = np.fmax(np.fmax(self.A, self.B), self.C)


def valid_boxes(boxes):
    """(n,) bool: every bound finite and lo <= hi on every axis"""
    b = np.asarray(boxes, F).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        return np.isfinite(b[:, [0, 1, 2, 4, 5, 6]]).all(-1) & (b[:, 0:3] <= b[:, 4:7]).all(-1)


def surviving_pairs(tris, boxes, cull_mask=0xFF, chunk=1 << 24):
    """(box index, triangle index) arrays of the pairs of valid boxes and finite triangles of admitted instances that step 2 does not
    separate, in (box, inst, prim) order"""
    b = np.asarray(boxes, F).reshape(-1, 8)
    ok_t = tris.finite & tris.scene.admitted(cull_mask)
    ok_b = valid_boxes(b)
    bi, ti = [], []
    per = max(1, chunk // max(1, len(ok_t)))
    for k0 in range(0, len(b), per):
        lo, hi = b[k0:k0 + per, None, 0:3], b[k0:k0 + per, None, 4:7]
        with np.errstate(invalid="ignore"):
            sep = (tris.mn[None] > hi).any(-1) | (tris.mx[None] < lo).any(-1)
        i, t = np.nonzero(~sep & ok_t[None] & ok_b[k0:k0 + per, None])
        bi.append(i + k0); ti.append(t)
    return (np.concatenate(bi), np.concatenate(ti)) if bi else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def _axes(lo, hi, A, B, C, f32):
    """steps 3 to 5 on pair arrays (3, m): yields (p0, p1, p2, r, scale) per axis — the projections, the box radius, and the 1-norm of the
    axis.  f32: binary32 with the canonical operation order; else binary64."""
    if f32:
        half = F(0.5)
        dot, cross = dot3, cross3
    else:
        half = 0.5
        lo, hi, A, B, C = (x.astype(np.float64) for x in (lo, hi, A, B, C))
        dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]   # noqa: E731
        cross = lambda a, b: (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])   # noqa: E731
    c = half * lo + half * hi
    h = half * hi - half * lo
    v = [A - c, B - c, C - c]
    f = [v[1] - v[0], v[2] - v[1], v[0] - v[2]]
    for e in f:
        af = np.abs(e)
        yield tuple(w[2] * e[1] - w[1] * e[2] for w in v) + (h[1] * af[2] + h[2] * af[1], af[1] + af[2])
        yield tuple(w[0] * e[2] - w[2] * e[0] for w in v) + (h[0] * af[2] + h[2] * af[0], af[0] + af[2])
        yield tuple(w[1] * e[0] - w[0] * e[1] for w in v) + (h[0] * af[1] + h[1] * af[0], af[0] + af[1])
    n = cross(tuple(f[0]), tuple(f[1]))
    an = tuple(np.abs(x) for x in n)
    d = dot(n, tuple(v[0]))
    yield d, d, d, dot(tuple(h), an), an[0] + an[1] + an[2]


def _pair_arrays(tris, boxes, bi, ti):
    b = np.asarray(boxes, F).reshape(-1, 8)
    return b[bi, 0:3].T, b[bi, 4:7].T, tris.A[ti].T, tris.B[ti].T, tris.C[ti].T


def candidates32(tris, boxes, bi, ti):
    """(pairs,) bool: the canonical predicate does not separate the pair (steps 3 to 5; step 2 is surviving_pairs')"""
    sep = np.zeros(len(bi), bool)
    with np.errstate(all="ignore"):
        for p0, p1, p2, r, _ in _axes(*_pair_arrays(tris, boxes, bi, ti), f32=True):
            sep |= (np.fmin(np.fmin(p0, p1), p2) > r) | (np.fmax(np.fmax(p0, p1), p2) < -r)
    return ~sep


def separation64(tris, boxes, bi, ti):
    """(pairs,) float64: the largest gap over the thirteen axes (step 2's three included), each relative to the magnitudes involved:
    > 0 separated by that much, <= 0 not separated, penetrating by that much.  The scale of an axis is the first-order size of what
    binary32 rounds on it.  With M the largest coordinate magnitude of the pair, V the largest centred coordinate (h included), F the
    largest edge component and |L|_1 the 1-norm of the axis: a box axis compares coordinates (scale M); a projection on e_i x f_j is a
    sum of products of an edge component and a centred coordinate, which carries the rounding of the centre c (terms of size M), and the
    edge components carry the rounding of the centred coordinates they are differences of (scale |L|_1 M + V V); the plane's normal is a
    product of two such edges (scale |L|_1 M + F V V).  An axis of zero norm (zero-area triangles) separates nothing."""
    lo, hi, A, B, C = (x.astype(np.float64) for x in _pair_arrays(tris, boxes, bi, ti))
    M = np.maximum(np.maximum(np.abs(A).max(0), np.abs(B).max(0)), np.maximum(np.abs(C).max(0), np.maximum(np.abs(lo).max(0), np.abs(hi).max(0))))
    M = np.where(M > 0, M, 1.0)
    c, h = 0.5 * lo + 0.5 * hi, 0.5 * hi - 0.5 * lo
    V = np.maximum(np.maximum(np.abs(A - c).max(0), np.abs(B - c).max(0)), np.maximum(np.abs(C - c).max(0), h.max(0)))
    Fm = np.maximum(np.abs(B - A).max(0), np.maximum(np.abs(C - B).max(0), np.abs(A - C).max(0)))
    s = np.full(len(bi), -np.inf)
    for k in range(3):
        mn, mx = np.minimum(np.minimum(A[k], B[k]), C[k]), np.maximum(np.maximum(A[k], B[k]), C[k])
        s = np.maximum(s, np.maximum(mn - hi[k], lo[k] - mx) / M)
    with np.errstate(all="ignore"):
        for k, (p0, p1, p2, r, norm) in enumerate(_axes(lo, hi, A, B, C, f32=False)):
            gap = np.maximum(np.minimum(np.minimum(p0, p1), p2) - r, -r - np.maximum(np.maximum(p0, p1), p2))
            scale = norm * M + (V * V if k < 9 else Fm * V * V)
            s = np.maximum(s, np.where(norm > 0, gap / np.where(scale > 0, scale, 1.0), -np.inf))
    return s


def rows(scene, n, bi, ti, keep, max_ids):
    """counts (n,) uint32 and ids (n, max_ids, 2) int32 of the kept pairs: the max_ids smallest (inst, prim) of every box ascending (Scene
    orders its triangles by (inst, prim)), (-1, -1) past the last"""
    bi, ti = bi[keep], ti[keep]
    per_box = np.bincount(bi, minlength=n).astype(np.int64)
    counts = per_box.astype(np.uint32)
    ids = np.full((n, max_ids, 2), -1, np.int32)
    if max_ids and len(bi):
        order = np.lexsort((ti, bi))
        bi, ti = bi[order], ti[order]
        first = np.cumsum(per_box) - per_box
        rank = np.arange(len(bi)) - first[bi]
        take = rank < max_ids
        ids[bi[take], rank[take], 0] = scene.inst[ti[take]]
        ids[bi[take], rank[take], 1] = scene.prim[ti[take]]
    return counts, ids


def brute32(scene, boxes, cull_mask=0xFF, max_ids=16, tris=None):
    """counts (n,) uint32 and ids (n, max_ids, 2) int32 of the canonical binary32 predicate over all (box, instance, triangle) pairs"""
    tris = tris or Triangles(scene)
    n = len(np.asarray(boxes, F).reshape(-1, 8))
    bi, ti = surviving_pairs(tris, boxes, cull_mask)
    return rows(scene, n, bi, ti, candidates32(tris, boxes, bi, ti), max_ids)


def brute64(scene, boxes, cull_mask=0xFF, max_ids=16, tris=None):
    """the same in binary64 on the same binary32 A, B, C, lo, hi (a pair is a candidate when its separation is <= 0)"""
    tris = tris or Triangles(scene)
    n = len(np.asarray(boxes, F).reshape(-1, 8))
    bi, ti = surviving_pairs(tris, boxes, cull_mask)
    return rows(scene, n, bi, ti, separation64(tris, boxes, bi, ti) <= 0, max_ids)
