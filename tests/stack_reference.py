"""CPU model of the traversal stack's peak: how many entries a walk kernel holds at most for one query.

Plain Python in binary64 over a snapshot in tree_reference.py's layout (RtContext.debug_snapshot, or tree_reference.link_meshes
over api.host_blas without a GPU).  One query is walked through the TLAS and the BLAS of every instance it enters, the way the
kernels in csrc/kernels*.hip/.inc do, and the largest stack pointer `sp` is returned.  The model counts what the kernels count:

  stk[0] = REF_DONE, sp = 1            the bottom sentinel, written when the query starts
  push(the other child)                at every interior node, TLAS or BLAS, whose two children are both entered
  push(REF_MARK)                       when a TLAS leaf is entered (the leave-instance marker), before the BLAS root becomes current
  pop()                                at a node none of whose children is entered, after a leaf, at REF_MARK

The node being visited is held in a register (`cur`), not on the stack.  An entry lies in LDS while its index is below STACK2_LDS
(kernels.hip: RT_STACK2_LDS) and in the per-thread spill area behind it: a walk spills if and only if its peak exceeds STACK2_LDS.

Three descent rules, each as its source states it:
  NEAR   trace_body / k_query_hits / inside_body / sweep_body / beam_body: `swap = t1 < t0; push(swap ? ch.x : ch.y); cur = swap ?
         ch.y : ch.x`: the child whose slab entry is nearer first, ties to child 0.  Queries: rays, and sweeps (boxes widened by r).
         The product library's shadow rays walk trace_body too (MODE_SHADOW, any hit): the same rule.  Two things the model does not
         restate: an entry record (camera tiles, the light's cube) seeds the walk with up to ENTRY_WORDS words, under ENTRY_REVERSE in
         the opposite order, and k_beam walks the rays of a pixel together, ordering children by the beam's entry; tests that go
         through them take a larger margin.  (beam_shadow_body, alt library only, visits the child that reaches farther from the
         light first: not modelled.)
  BOUND  nearest_body: `swap = b1 < b0` on the squared distance from the point to the child's box: the smaller bound first; a child
         is entered while its bound does not exceed the search radius squared.
  FIRST  overlap_body: `push(Q1.w); cur = Q1.z`: child 0 first.  A child is entered if its box touches the query box.

The model establishes PREMISES ("this input reaches depth d"), never results: it dequantises the planes in binary64 and tests them
without the kernels' slack terms, so a tie or a plane within rounding of the query may go the other way.  Two figures come back:

  first   the peak up to the first BLAS leaf the walk reaches.  Nothing prunes before the first triangle is tested (best_t is the
          ray's tmax, best the radius squared), so up to the order of exact ties this is what the kernel does: a LOWER bound of its peak.
  full    the peak of the whole walk with nothing pruned (an all-hits walk): exact for all-hits, inside and overlap walks, an UPPER
          bound for closest-hit, any-hit, closest-point and sweep walks.

Tests assert premises on `first` with a margin (tests/test_stack_spill.py)."""
import re
import os

import numpy as np

NEAR, BOUND, FIRST = "near", "bound", "first"
_DONE, _MARK = "done", "mark"


def stack2_lds():
    """RT_STACK2_LDS as kernels.hip defines it"""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "vulkan_raytracing_amd", "csrc", "kernels.hip")
    m = re.findall(r"^#define RT_STACK2_LDS (\d+)", open(src).read(), re.M)
    assert len(m) == 1, m
    return int(m[0])


class Ray:
    """(o, d, tmin, tmax), optionally a sphere of radius r swept along it: rule NEAR"""
    rule = NEAR

    def __init__(self, o, d, tmin=0.0, tmax=np.inf, r=0.0):
        self.o, self.d = [float(x) for x in o], [float(x) for x in d]
        self.tmin, self.tmax, self.r = float(tmin), float(tmax), float(r)

    def into(self, M, scale):
        o = [M[a][0] * self.o[0] + M[a][1] * self.o[1] + M[a][2] * self.o[2] + M[a][3] for a in range(3)]
        d = [M[a][0] * self.d[0] + M[a][1] * self.d[1] + M[a][2] * self.d[2] for a in range(3)]
        return Ray(o, d, self.tmin, self.tmax, self.r / scale if self.r else 0.0)      # (t is preserved)

    def test(self, lo, hi):
        tn, tf = self.tmin, self.tmax
        for a in range(3):
            l, h, o, d = lo[a] - self.r, hi[a] + self.r, self.o[a], self.d[a]
            if d == 0.0:
                if o < l or o > h:
                    return False, 0.0
                continue
            t1, t2 = (l - o) / d, (h - o) / d
            if t1 > t2:
                t1, t2 = t2, t1
            tn, tf = max(tn, t1), min(tf, t2)
        return tn <= tf, tn


class Point:
    """a point and a search radius (world units): rule BOUND"""
    rule = BOUND

    def __init__(self, p, radius=np.inf, scale2=1.0):
        self.p, self.radius, self.scale2 = [float(x) for x in p], float(radius), float(scale2)

    def into(self, M, scale):
        p = [M[a][0] * self.p[0] + M[a][1] * self.p[1] + M[a][2] * self.p[2] + M[a][3] for a in range(3)]
        return Point(p, self.radius, scale * scale)       # (object-space distances times the instance's scale are world distances)

    def test(self, lo, hi):
        d2 = 0.0
        for a in range(3):
            d = max(lo[a] - self.p[a], self.p[a] - hi[a], 0.0)
            d2 += d * d
        d2 *= self.scale2
        return not (d2 > self.radius * self.radius), d2


class Box:
    """an axis-aligned query box (world space): rule FIRST.  In an instance: the bounds of its eight transformed corners."""
    rule = FIRST

    def __init__(self, lo, hi):
        self.lo, self.hi = [float(x) for x in lo], [float(x) for x in hi]

    def into(self, M, scale):
        c = [[M[a][0] * x + M[a][1] * y + M[a][2] * z + M[a][3] for a in range(3)]
             for x in (self.lo[0], self.hi[0]) for y in (self.lo[1], self.hi[1]) for z in (self.lo[2], self.hi[2])]
        return Box([min(p[a] for p in c) for a in range(3)], [max(p[a] for p in c) for a in range(3)])

    def test(self, lo, hi):
        return all(self.lo[a] <= hi[a] and lo[a] <= self.hi[a] for a in range(3)), 0.0


class StackModel:
    def __init__(self, snap, frame=0):
        self.snap = snap
        self.base = int(snap["tlas_base"])
        self.root = self.base + frame * (int(snap["tlas_stride"]) if int(snap["batch_k"]) > 1 else 0)
        self.t_lo = [float(x) for x in np.asarray(snap["tlas_q_lo"], np.float32)]
        self.t_s = [float(x) for x in np.asarray(snap["tlas_q_scale"], np.float32)]
        self.tn_w, self.tn_c = snap["tlas_nodes"]["w"].tolist(), snap["tlas_nodes"]["child"].tolist()
        self.bn_w = self.bn_c = None
        inst = snap["instances"]
        self.w2o = inst["w2o"].astype(np.float64).reshape(-1, 3, 4).tolist()
        o2w = inst["o2w"].astype(np.float64).reshape(-1, 3, 4)[:, :, :3]
        self.scale = np.abs(np.linalg.det(o2w)) ** (1.0 / 3.0)          # (the tests' instances are rigid or uniformly scaled up to a shear)
        self.i_lo, self.i_s = inst["q_lo"].astype(np.float64).tolist(), inst["q_scale"].astype(np.float64).tolist()
        self.i_root = inst["blas_root"].tolist()

    def _blas(self):
        if self.bn_w is None:
            self.bn_w, self.bn_c = self.snap["blas_nodes"]["w"].tolist(), self.snap["blas_nodes"]["child"].tolist()
        return self.bn_w, self.bn_c

    def peak(self, query, full=False, blas_only=None):
        """the peak of `query` (Ray, Point or Box, world space).  Returns (first, full) with full = None unless asked for.
        blas_only = i: the walk of instance i's BLAS alone, counting its pending entries only (no sentinel, no marker)."""
        bn_w, bn_c = self._blas()
        rule = query.rule
        stack = [_DONE]
        peak = first = None
        if blas_only is None:
            cur, cur_inst, q, lo0, s0 = self.root, -1, query, self.t_lo, self.t_s
        else:
            stack = []
            cur_inst = blas_only
            cur, q, lo0, s0 = self.i_root[cur_inst], query.into(self.w2o[cur_inst], self.scale[cur_inst]), self.i_lo[cur_inst], self.i_s[cur_inst]
        peak = len(stack)
        while True:
            if cur is _DONE:
                break
            if cur is _MARK:
                cur_inst, q, lo0, s0 = -1, query, self.t_lo, self.t_s
                cur = stack.pop()
                continue
            if cur >= 0:
                if cur_inst < 0:
                    w, ch = self.tn_w[cur - self.base], self.tn_c[cur - self.base]
                else:
                    w, ch = bn_w[cur], bn_c[cur]
                hit, key = [False, False], [0.0, 0.0]
                for k in range(2):
                    ws = w[3 * k:3 * k + 3]
                    if any((x & 0xFFFF) > (x >> 16) for x in ws):
                        continue                                            # an inverted box: no child
                    lo = [lo0[a] + (ws[a] & 0xFFFF) * s0[a] for a in range(3)]
                    hi = [lo0[a] + (ws[a] >> 16) * s0[a] for a in range(3)]
                    hit[k], key[k] = q.test(lo, hi)
                if hit[0] and hit[1]:
                    swap = rule != FIRST and key[1] < key[0]
                    stack.append(ch[0] if swap else ch[1])
                    peak = max(peak, len(stack))
                    cur = ch[1] if swap else ch[0]
                elif hit[0]:
                    cur = ch[0]
                elif hit[1]:
                    cur = ch[1]
                else:
                    if not stack:
                        break
                    cur = stack.pop()
                continue
            if cur_inst < 0:                                                # TLAS leaf: enter the instance
                cur_inst = ~cur
                stack.append(_MARK)
                peak = max(peak, len(stack))
                cur, q, lo0, s0 = self.i_root[cur_inst], query.into(self.w2o[cur_inst], self.scale[cur_inst]), self.i_lo[cur_inst], self.i_s[cur_inst]
                continue
            if first is None:                                               # BLAS leaf
                first = peak
                if not full:
                    return first, None
            if not stack:
                break
            cur = stack.pop()
        return (peak if first is None else first), (peak if full else None)

    def first(self, query):
        return self.peak(query)[0]

    def full(self, query):
        return self.peak(query, full=True)[1]


def rays_of(rays8, r=None):
    """Ray objects of (n, 8) rows (o, tmin, d, tmax); sweeps: rows (o, r, d, tmax) with the radius in column 3"""
    rays8 = np.asarray(rays8, np.float64)
    if r is None:
        return [Ray(x[0:3], x[4:7], x[3], x[7]) for x in rays8]
    return [Ray(x[0:3], x[4:7], 0.0, x[7], r=x[3]) for x in rays8]


def host_snapshot(meshes, transforms=None):
    """a snapshot of host-built trees without a GPU: meshes is a list of (verts6, idx); one instance per mesh (see link_meshes)"""
    from tests import tree_reference as tr
    from vulkan_raytracing_amd import api
    parts = []
    for v, ix in meshes:
        rc, b = api.host_blas(v, ix)
        assert rc == 0
        parts.append((v, ix, b["nodes"], b["packets"], b["q_lo"], b["q_scale"], tree_levels(b["nodes"])))
    return tr.link_meshes(parts, transforms)[0]


def tree_levels(nodes, root=0):
    """interior levels of a tree with local links"""
    ch = nodes["child"].astype(np.int64)
    cur, levels = np.array([root]), 0
    while len(cur):
        levels += 1
        nxt = np.unique(ch[cur].reshape(-1))
        cur = nxt[nxt >= 0]
    return levels
