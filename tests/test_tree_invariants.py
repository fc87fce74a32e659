"""Every tree the kernels walk, checked node by node: each box on the path from a root to a triangle contains that triangle, in the
fixed-point planes the kernels read ("The contract of every tree producer").

rt_debug_snapshot copies the linked BLAS nodes, a context's TLAS region, the packets, the instance records, the mesh table, the vertex
and index buffers and the frontier boxes to the host; tests/tree_reference.py visits every node, packet and instance once and decides
every comparison exactly.  The ray tests sample a tree with a few ten thousand rays and miss a box that is one quantum too tight; this
check is deterministic and complete.  Every test asserts zero violations of every kind AND that the walk reached what it should."""
import os
import re
import time
from fractions import Fraction

import numpy as np
import pytest

from tests import scenes, tree_reference as tr
from vulkan_raytracing_amd import RtContext, api, host
from vulkan_raytracing_amd.api import INSTANCE_DTYPE

ROOT = scenes.ROOT
RES = scenes.RES
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
IDENTITY = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)


def clean(viol):
    return {k: v for k, v in viol.items() if v}


# ---- shapes ---------------------------------------------------------------------------------------------------------------------------

def _mesh(pos, tri):
    """(verts6 (nv, 6) float32 with a constant normal, idx (3 nt,) uint32)"""
    pos = np.asarray(pos, np.float32)
    v = np.zeros((len(pos), 6), np.float32)
    v[:, :3] = pos
    v[:, 5] = 1.0
    return v, np.asarray(tri, np.uint32).reshape(-1)


def _obj(name):
    g = host.SceneGeometry([os.path.join(RES, name + ".obj")])
    return g.verts.reshape(-1, 6).copy(), g.idx.copy()


def _grid(n, z):
    """n x n quads in the plane z = const"""
    x, y = np.meshgrid(np.linspace(-1.3, 2.1, n + 1), np.linspace(0.2, 3.3, n + 1), indexing="ij")
    pos = np.stack([x.ravel(), y.ravel(), np.full(x.size, z)], axis=1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).ravel()
    tri = np.stack([a, a + 1, a + n + 2, a, a + n + 2, a + n + 1], axis=1).reshape(-1, 3)
    return _mesh(pos, tri)


def soup():
    """the degenerate soup of test_gpu_parity.test_device_builders_on_degenerate_soup: 40 distinct positions among 320 vertices, a
    coplanar patch, coincident and zero-area triangles, needles, exact duplicates"""
    rng = np.random.default_rng(11)
    pts = np.repeat(rng.normal(size=(40, 3)), 8, axis=0)
    pts[:80, 2] = 0.25
    tri = rng.integers(0, len(pts), size=(700, 3))
    tri[:50] = tri[50:100]
    return _mesh(pts, tri)


def shapes():
    rng = np.random.default_rng(2024)
    out = {"teapot": _obj("teapot"), "cube": _obj("cube"), "soup": soup()}
    v, i = _obj("teapot")
    far = v.copy()
    far[:, :3] = (v[:, :3] * np.float32(0.01) + np.array([1000, -2000, 500], np.float32)).astype(np.float32)   # the quantum is far below the ulp of the coordinates
    out["teapot_far"] = (far, i)
    out["flat"] = _grid(20, 0.75)                                           # q_scale = 1e-30 on z
    out["flat0"] = _grid(9, 0.0)                                            # ... with q_lo = -4e-30
    t = rng.uniform(-3, 5, 200)
    out["line"] = _mesh(t[:, None] * np.array([1.0, 2.0, -0.5]) + np.array([0.1, 0.0, 0.0]), rng.integers(0, 200, size=(300, 3)))
    c = np.array([1.0, 1.0, 1.0]) + rng.uniform(-1e-3, 1e-3, size=(4096, 1, 3)) + rng.uniform(-2e-5, 2e-5, size=(4096, 3, 3))
    pos = np.concatenate([c.reshape(-1, 3), [[1e4, 1.0, 1.0], [1e4, 2.0, 1.0], [1e4, 1.0, 3.0]]])
    out["cluster"] = _mesh(pos, np.arange(len(pos)).reshape(-1, 3))         # 4 k tiny triangles + one 1e4 away: boxes collapse inside one quantum
    for n in (9, 8, 7):                                                     # 8: the device builder's lower limit; 7: falls back to the host path
        out["tri%d" % n] = _mesh(rng.normal(size=(3 * n, 3)), np.arange(3 * n).reshape(-1, 3))
    return out


def pack(meshes, empty_last=False):
    """(verts, idx, ranges) of one scene holding every mesh of the list; empty_last appends a mesh without triangles"""
    verts, idx, ranges, nf, ni = [], [], [], 0, 0
    for v, i in meshes:
        ranges.append((nf, ni, len(i) // 3))
        verts.append(v.reshape(-1)); idx.append(i)
        nf += v.size; ni += len(i)
    if empty_last:
        ranges.append((0, ni, 0))
    return np.concatenate(verts), np.concatenate(idx), ranges


def one_instance_each(n, shift=0.0):
    inst = np.zeros(n, INSTANCE_DTYPE)
    for m in range(n):
        M = IDENTITY.copy()
        M[3] = shift * m
        inst[m] = host.make_instance(M, m, m)
    return inst


def check(snap, inst_mesh, prim_counts, n_reached=None, frames=1):
    """zero violations of every kind, every packet of every mesh and every instance with triangles reached; returns what was reached"""
    viol, reached = tr.validate(snap, inst_mesh)
    assert clean(viol) == {}, (clean(viol), reached)
    assert reached["packets"] == {m: pc for m, pc in enumerate(prim_counts) if pc}, reached
    per_frame = len(inst_mesh) // frames
    want = n_reached if n_reached is not None else int(sum(prim_counts[m] > 0 for m in np.asarray(inst_mesh)[:per_frame]))
    assert reached["instances"] == [want] * frames, (reached["instances"], want)
    return reached


# ---- CPU: the validator can fail ------------------------------------------------------------------------------------------------------

def synthetic(void=None, leak=False, bad_tri=False):
    """bad_tri: triangle 5 of mesh 0 (leaf D, coincident with triangle 4) gets a NaN into the y of its three vertices and is INACTIVE
    as the library leaves it — its packet holds the NaN, its leaf keeps its link under inverted planes, bounds and frame are those of
    the other five.  void: a record (of mesh 0 or 1) made VOID as the library leaves it — a NaN in its transform, mask word 0, no box in its leaf, out
    of the bounds; leak: its box, had the NaN been dropped and a 1e37 translation kept, counted into the bounds all the same.
    Two meshes with triangles, one without, five instances and a two-frame batch, quantised by the documented rule (lower planes
    rounded down, upper planes up, one whole quantum further out).  Mesh 0: node 0 -> (node 1: leaves A = packets 0, 1 and B = 2, 3;
    node 2: leaves C = 4 and D = 5, two coincident triangles).  Mesh 1: one leaf of two triangles under a synthetic single-child root.
    Per frame: instances 0, 2 of mesh 0, 1, 3 of mesh 1, 4 of the empty mesh 2; TLAS ((0, 1), (2, (3, 4))), the leaf of instance 4
    drawn with the box of instance 3 (the validator does not look at the boxes of empty meshes; the defects below use it)."""
    rng = np.random.default_rng(7)
    t0 = rng.uniform(0, 1, size=(6, 3, 3))
    t0[4:] += [3.0, 0.5, -0.25]
    t0[5] = t0[4]
    t1 = rng.uniform(-2, -1, size=(2, 3, 3))
    if bad_tri:
        t0[5, :, 1] = np.nan
    m0, m1 = _mesh(t0.reshape(-1, 3), np.arange(18).reshape(-1, 3)), _mesh(t1.reshape(-1, 3), np.arange(6).reshape(-1, 3))
    verts, idx, ranges = pack([m0, m1], empty_last=True)
    packets = np.zeros(8, api.TRI_PACKET_DTYPE)
    meshes = np.zeros(3, api.TLAS_MESH_DTYPE)
    nodes, cover = [], []
    for m, ((v, i), topo, nn, nt) in enumerate([(m0, (([0, 1], [2, 3]), ([4], [5])), 0, 0), (m1, ([0, 1],), 4, 6)]):   # mesh 1 starts on a line of four nodes
        P = v[:, :3][i.astype(np.int64)].reshape(-1, 3, 3)
        lo, hi = tr.active_bounds(P)
        q_lo, q_s = tr.quant_params(lo, hi)
        box = lambda leaf: tr.active_bounds(P[leaf]) if tr.active_triangles(P[leaf]).any() else None
        nd = tr.build_tree(topo, box, lambda leaf: ((leaf[0] + nt) << 3) | (len(leaf) - 1), q_lo, q_s, margin=1, first=nn, keep_links=True)
        if len(nd) == 1 and len(topo) == 1:
            nd[0]["child"][1] = nd[0]["child"][0]                                # (the absent child of the synthetic root repeats its sibling's link)
        for p in range(len(P)):
            packets[nt + p] = (P[p, 0], P[p, 1] - P[p, 0], P[p, 2] - P[p, 0], p, (0, 0))
        first_cover = len(cover)
        for k in range(2):                                                     # frontier: the boxes of the root's children, dequantised and padded
            w = nd[0]["w"][3 * k:3 * k + 3].astype(np.int64)
            if ((w & 0xFFFF) <= (w >> 16)).all():
                blo = (q_lo.astype(np.float64) + (w & 0xFFFF) * q_s.astype(np.float64)).astype(np.float32)
                bhi = (q_lo.astype(np.float64) + (w >> 16) * q_s.astype(np.float64)).astype(np.float32)
                pad = np.float32(1e-6) * (np.abs(blo) + np.abs(bhi))
                cover.append(np.concatenate([blo - pad, bhi + pad]))
        meshes[m] = (nn, 0, ranges[m][0], ranges[m][1], first_cover, len(cover) - first_cover, len(P), 1, 2 if m == 0 else 1, q_lo, q_s, lo, hi)
        nodes.append(nd)
    meshes[2] = (8, 0, 0, ranges[2][1], len(cover), 0, 0, 1, 0, (0, 0, 0), (1, 1, 1), (3e38,) * 3, (-3e38,) * 3)
    blas = np.zeros(8, api.NODEQ_DTYPE)
    blas[0:3], blas[3], blas[4], blas[5:] = nodes[0], nodes[0][0], nodes[1][0], nodes[0][0]          # (slots 3 and 5..7: filler, never referenced)
    n, K = 5, 2
    inst_mesh = np.array([0, 1, 0, 1, 2] * K)
    inst = np.zeros(n * K, api.INSTANCE_DEV_DTYPE)
    boxes = []
    for r in range(n * K):
        k, j = divmod(r, n)
        a = 0.7 * j + 0.4 * k
        s = 0.5 + 0.25 * j
        M = np.array([[s * np.cos(a), 0, s * np.sin(a), 6.0 * j - 3.0 * k], [0.2 * s, s, 0, 1.5 * k], [-s * np.sin(a), 0, -s * np.cos(a), 2.0 * j]], np.float32)   # sheared, mirrored
        me = meshes[inst_mesh[r]]
        inst[r]["o2w"] = M.reshape(12)
        for f in ("blas_root", "first_float", "first_index", "cover_first", "cover_count", "q_lo", "q_scale"):
            inst[r][f] = me[f]
        inst[r]["mask"] = 0xFF if me["prim_count"] else 0
        boxes.append(tr.world_box(M, me["lo"], me["hi"]) if me["prim_count"] else None)
    for k in range(K):
        boxes[k * n + 4] = boxes[k * n + 3]
    valid = [b for b in boxes if b is not None]
    if void is not None:
        inst[void]["o2w"][5] = np.nan
        inst[void]["mask"] = 0
        boxes[void] = None
        valid = [b for b in boxes if b is not None] + ([(np.full(3, 1e37), np.full(3, 1.0001e37))] if leak else [])
    t_lo, t_s = tr.quant_params(np.min([b[0] for b in valid], axis=0), np.max([b[1] for b in valid], axis=0))
    base, stride = 8 + 2048, 4
    tlas = np.concatenate([tr.build_tree(((0, 1), (2, (3, 4))), lambda j, k=k: boxes[k * n + j], lambda j, k=k: k * n + j, t_lo, t_s, 1, base + k * stride)
                           for k in range(K)])
    snap = {"n_blas_nodes": 8, "tlas_base": base, "tlas_node_count": stride, "tlas_stride": stride, "batch_k": K, "inst_per_frame": n,
            "tlas_q_lo": t_lo, "tlas_q_scale": t_s, "blas_nodes": blas, "tlas_nodes": tlas, "packets": packets, "instances": inst, "meshes": meshes,
            "verts": verts, "idx": idx, "cover_boxes": np.array(cover, np.float32).reshape(-1, 6)}
    return snap, inst_mesh


def _plane_below(x, q_lo, q_s):
    """the nearest plane strictly below x"""
    return int(np.ceil((float(x) - float(q_lo)) / float(q_s))) - 1


def _plane_above(x, q_lo, q_s):
    return int(np.floor((float(x) - float(q_lo)) / float(q_s))) + 1


def _set_plane(node, k, axis, lo=None, hi=None):
    w = int(node["w"][3 * k + axis])
    l, h = w & 0xFFFF, w >> 16
    node["w"][3 * k + axis] = (l if lo is None else lo) | ((h if hi is None else hi) << 16)


def _d_upper(s):
    m = s["meshes"][0]
    x = s["verts"].reshape(-1, 6)[:6, 0].max()                                  # leaf A = triangles 0, 1 = vertices 0..5
    _set_plane(s["blas_nodes"][1], 0, 0, hi=_plane_below(x, m["q_lo"][0], m["q_scale"][0]))


def _d_lower(s):
    m = s["meshes"][0]
    y = s["verts"].reshape(-1, 6)[6:12, 1].min()                                # leaf B
    _set_plane(s["blas_nodes"][1], 1, 1, lo=_plane_above(y, m["q_lo"][1], m["q_scale"][1]))


def _d_ancestor(s):
    s["blas_nodes"][2]["child"][1] = 0


def _d_packet_twice(s):
    s["blas_nodes"][2]["child"][0] = ~((4 << 3) | 1)                            # leaf C grows over packet 5 (the coincident triangle of leaf D)


def _d_packet_none(s):
    s["blas_nodes"][1]["child"][0] = ~((0 << 3) | 0)                            # leaf A shrinks to packet 0


def _d_e1(s):
    s["packets"][2]["e1"][1] = np.nextafter(s["packets"][2]["e1"][1], np.float32(np.inf))


def _d_tlas_box(s):
    m = s["meshes"][0]
    lo, hi = tr.world_box(s["instances"][0]["o2w"], m["lo"], m["hi"])
    _set_plane(s["tlas_nodes"][1], 0, 1, hi=_plane_below(hi[1], s["tlas_q_lo"][1], s["tlas_q_scale"][1]))   # node 1 of frame 0 = (0, 1)


def _d_inst_twice(s):
    s["tlas_nodes"][3]["child"][1] = ~3                                         # node 3 = (3, 4): the leaf of the empty instance 4 names 3


def _d_inst_none(s):
    nd = s["tlas_nodes"][3]
    nd["w"][0:3] = tr.INVERTED
    nd["child"][0] = nd["child"][1]


def _d_frontier(s):
    s["meshes"][0]["cover_count"] -= 1
    s["instances"]["cover_count"][[0, 2, 5, 7]] -= 1


def _d_q_scale(s):
    s["instances"][2]["q_scale"][1] = np.nextafter(s["instances"][2]["q_scale"][1], np.float32(np.inf))


def _d_frame(s):
    s["tlas_nodes"][4 + 3]["child"][1] = ~4                                     # frame 1's leaf of its empty instance 9 names record 4 of frame 0


def _d_void_leaked(s):
    return synthetic(void=2, leak=True)[0]                                      # record 2 is void, and the bounds were taken as if it were not


def _d_box_none(s):
    s["tlas_nodes"][1]["w"][0:3] = 0xFFFFFFFF                                   # node 1 = (0, 1): the good record 0 drawn with BOX_NONE (the last quantum)


def _d_void_mask(s):
    s = synthetic(void=2)[0]                                                    # record 2 is void and out of the bounds, but its mask stayed
    s["instances"][2]["mask"] = 0xFF
    return s


def _d_root_order(s):
    s["instances"]["mask"][[0, 1]] = 0                                          # records 0 and 1 masked out by the caller, their subtree dropped ...
    nd = s["tlas_nodes"][0]                                                     # ... as the FIRST child of frame 0's root
    nd["w"][0:3] = tr.INVERTED
    nd["child"][0] = nd["child"][1]


def _bad(seed):
    """the seed applied to the snapshot with the inactive triangle"""
    def f(_):
        s = synthetic(bad_tri=True)[0]
        seed(s)
        return s
    return f


def _d_frame_inf(s):
    s["meshes"][0]["q_scale"][1] = np.inf                                        # what one infinite coordinate made of the frame before the contract
    s["instances"]["q_scale"][[0, 2, 5, 7], 1] = np.inf


def _d_bounds(s):
    s["meshes"][0]["hi"][0] = np.nextafter(s["meshes"][0]["hi"][0], np.float32(np.inf))   # one ulp beyond the active triangles


def _d_blas_frame(s):
    q = np.nextafter(s["meshes"][0]["q_lo"][2], np.float32(-np.inf))
    s["meshes"][0]["q_lo"][2] = q
    s["instances"]["q_lo"][[0, 2, 5, 7], 2] = q


def _d_active_absent(s):
    s["blas_nodes"][2]["w"][0:3] = tr.INVERTED                                   # leaf C holds the active triangle 4: inverted planes, its own link


DEFECTS = [("an upper plane one quantum below a vertex", _d_upper, "blas_hi"), ("a lower plane one quantum above a vertex", _d_lower, "blas_lo"),
           ("a link redirected to an ancestor", _d_ancestor, "blas_node_twice"), ("a packet in two leaves", _d_packet_twice, "packet_twice"),
           ("a packet in no leaf", _d_packet_none, "packet_unreached"), ("e1 off by one ulp", _d_e1, "packet_bits"),
           ("a TLAS leaf box shrunk below a corner", _d_tlas_box, "tlas_containment"), ("an instance in two leaves", _d_inst_twice, "instance_twice"),
           ("an instance with triangles in no leaf", _d_inst_none, "instance_unreached"), ("a frontier box removed", _d_frontier, "frontier"),
           ("InstanceDev.q_scale one ulp off the mesh table", _d_q_scale, "record_fields"), ("a leaf of frame 1 naming a record of frame 0", _d_frame, "tlas_leaf_range"),
           ("a void record that leaked into the bounds", _d_void_leaked, "tlas_bounds"), ("a good record given BOX_NONE", _d_box_none, "tlas_containment"),
           ("a void record that kept its mask", _d_void_mask, "void_record"),
           ("the root's absent child in the first slot", _d_root_order, "tlas_root_order"),
           # bad vertices (appended: the ids of the cases above carry their position in the table)
           ("a frame that is not finite", _bad(_d_frame_inf), "blas_not_finite"), ("mesh bounds one ulp beyond the active triangles", _bad(_d_bounds), "blas_bounds"),
           ("q_lo one ulp off the documented frame", _bad(_d_blas_frame), "blas_frame"),
           ("an active triangle under inverted planes with a link of their own", _bad(_d_active_absent), "blas_inverted_link"),
           ("the same in a mesh without inactive triangles", _d_active_absent, "blas_inverted_link")]


def test_validator_accepts_a_clean_snapshot():
    snap, inst_mesh = synthetic()
    reached = check(snap, inst_mesh, [6, 2, 0], frames=2)
    assert reached["nodes"] == {0: 3, 1: 1} and reached["leaves"] == {0: 4, 1: 1} and reached["levels"] == {0: 2, 1: 1}
    assert reached["tlas_levels"] == [3, 3]


@pytest.mark.parametrize("name,seed,kind", DEFECTS, ids=[d[2] + str(i) for i, d in enumerate(DEFECTS)])
def test_validator_reports_each_seeded_defect_as_its_own_kind(name, seed, kind):
    snap, inst_mesh = synthetic()
    snap = seed(snap) or snap                                                   # (a seed may build the defective snapshot itself)
    viol, _ = tr.validate(snap, inst_mesh)
    assert list(clean(viol)) == [kind], (name, clean(viol))


def test_validator_accepts_an_inactive_triangle():
    """the same snapshot with triangle 5 of mesh 0 inactive as the library leaves it: reached or not, in no box, out of bounds and frame"""
    snap, inst_mesh = synthetic(bad_tri=True)
    viol, reached = tr.validate(snap, inst_mesh)
    assert clean(viol) == {} and reached["active"] == {0: 5, 1: 2} and reached["inactive"] == {0: 1, 1: 0} and reached["packets"][0] == 6, (clean(viol), reached)
    snap["blas_nodes"][2]["child"][1] = snap["blas_nodes"][2]["child"][0]       # ... and with its leaf dropped from the tree
    viol, reached = tr.validate(snap, inst_mesh)
    assert clean(viol) == {} and reached["active"] == {0: 5, 1: 2} and reached["packets"][0] == 5, (clean(viol), reached)


def test_validator_accepts_a_void_record():
    """the same snapshot with record 2 void as the library leaves it: mask word 0, no box, out of the bounds"""
    snap, inst_mesh = synthetic(void=2)
    viol, reached = tr.validate(snap, inst_mesh)
    assert clean(viol) == {} and reached["instances"] == [3, 4], (clean(viol), reached)


def _frac(x):
    return Fraction(float(x))


def test_exact_decisions_at_ties_and_tiny_scales():
    """cmp_plane decides in real arithmetic: coordinates on a plane, one binary64 ulp off it, and planes 1e-30 apart"""
    f = np.float32
    q_lo, s = float(f(0.75)), float(f(1e-30))
    assert tr.cmp_plane(0.75, 0.0, q_lo, 0, s).item() == 0 and tr.cmp_plane(0.75, 0.0, q_lo, 2, s).item() == -1
    assert tr.cmp_plane(0.0, 0.0, float(f(-4e-30)), 4, s).item() == 0          # fl32(4e-30) is exactly 4 fl32(1e-30)
    assert tr.cmp_plane(0.0, 0.0, float(f(-4e-30)), 3, s).item() == 1 and tr.cmp_plane(0.0, 0.0, float(f(-4e-30)), 5, s).item() == -1
    q_lo, s = float(f(1000.0)), float(f(9.5e-7))
    x = q_lo + 12345 * s                                                          # rounded in binary64: the exact sign comes from the fractions
    want = np.sign(_frac(x) - _frac(q_lo) - 12345 * _frac(s))
    assert tr.cmp_plane(x, 0.0, q_lo, 12345, s).item() == want
    assert tr.cmp_plane(np.nextafter(x, np.inf), 0.0, q_lo, 12345, s).item() == 1 and tr.cmp_plane(np.nextafter(x, -np.inf), 0.0, q_lo, 12345, s).item() == -1
    assert tr.cmp_plane(float(f(1e4)), float(f(3e-5)), q_lo, 65535, s).item() == 1   # v0 + e1 with 29 binary orders between them


# ---- CPU: real host trees -------------------------------------------------------------------------------------------------------------

def test_host_built_trees_hold_the_contract():
    """rt_debug_host_blas (rt_build_blas(blas_builder 0) + quantize_bvh2, no GPU) for every shape: zero violations, and nodes, leaves,
    depth and triangles reached as rt_debug_check_builders counts them"""
    names, parts = [], []
    for name, (v, i) in shapes().items():
        rc, hb = api.host_blas(v, i)
        assert rc == 0, name
        rc, st = api.check_builders(v, i)
        assert rc == 0 and st["violations"] == 0, (name, st)
        names.append(name)
        parts.append((v, i, hb["nodes"], hb["packets"], hb["q_lo"], hb["q_scale"], st["depth"], st))
    t0 = time.perf_counter()
    snap, inst_mesh = tr.link_meshes([p[:7] for p in parts])
    reached = check(snap, inst_mesh, [len(p[1]) // 3 for p in parts])
    print("validated %d host trees (%d packets) in %.2f s" % (len(parts), len(snap["packets"]), time.perf_counter() - t0))
    for m, (name, p) in enumerate(zip(names, parts)):
        st = p[7]
        assert (reached["nodes"][m], reached["leaves"][m], reached["levels"][m], reached["packets"][m]) == (st["nodes"], st["leaves"], st["depth"], st["reached"]), (name, st, reached)


def test_a_20k_triangle_mesh_validates_in_under_a_second(tmp_path):
    p = str(tmp_path / "s.obj")
    assert host.hlib().rth_write_armadillo_standin(p.encode(), 32) == 0           # 20 480 triangles
    g = host.SceneGeometry([p])
    rc, hb = api.host_blas(g.verts, g.idx)
    rc2, st = api.check_builders(g.verts, g.idx)
    assert rc == 0 and rc2 == 0
    snap, inst_mesh = tr.link_meshes([(g.verts, g.idx, hb["nodes"], hb["packets"], hb["q_lo"], hb["q_scale"], st["depth"])])
    t0 = time.perf_counter()
    reached = check(snap, inst_mesh, [len(g.idx) // 3])
    dt = time.perf_counter() - t0
    print("%d triangles validated in %.3f s" % (len(g.idx) // 3, dt))
    assert reached["packets"][0] == 20480 and dt < 1.0, dt


def test_snapshot_exports_and_argument_checks_without_a_device():
    assert "rt_debug_snapshot" in api.EXPORTS and "rt_debug_host_blas" in api.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    assert re.search(r"^int rt_debug_snapshot\(rt_ctx\* ctx, int what, void\* out, size_t capacity_bytes, size_t\* bytes\);", hdr, re.M)
    L = api.lib()
    assert L.rt_abi_version() == 7
    buf = np.zeros(64, np.uint64)
    assert L.rt_debug_snapshot(None, 0, api._p(buf), buf.nbytes, None) == RT_ERR_INVALID_ARGUMENT
    v, i = shapes()["tri9"]
    nodes, pk, out = np.zeros(16, api.NODEQ_DTYPE), np.zeros(9, api.TRI_PACKET_DTYPE), np.zeros(8, np.uint64)
    args = (api._p(v), v.size, api._p(i), i.size)
    assert L.rt_debug_host_blas(*args, api._p(nodes), nodes.nbytes, api._p(pk), pk.nbytes, api._p(out)) == 0 and int(out[1]) == 9
    assert L.rt_debug_host_blas(*args, api._p(nodes), nodes.nbytes, api._p(pk), pk.nbytes - 1, api._p(out)) == RT_ERR_INVALID_ARGUMENT   # short buffer
    assert L.rt_debug_host_blas(*args, api._p(nodes), 32, api._p(pk), pk.nbytes, api._p(out)) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_debug_host_blas(*args, None, nodes.nbytes, api._p(pk), pk.nbytes, api._p(out)) == RT_ERR_INVALID_ARGUMENT
    assert L.rt_debug_host_blas(api._p(v), 12, api._p(i), i.size, api._p(nodes), nodes.nbytes, api._p(pk), pk.nbytes, api._p(out)) == RT_ERR_INVALID_ARGUMENT


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

PATHS = [os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj")]
BUILDERS = ["host", "1", "2", "3"]   # rt_build_blas on the host (blas_builder 0), or on the device with RT_GPU_BVH_ALGO 1 / 2 / 3
_SHAPES = {}


def cached_shapes():
    if not _SHAPES:
        _SHAPES.update(shapes())
    return _SHAPES


def use_builder(c, builder, mp):
    if builder == "host":
        mp.delenv("RT_GPU_BVH_ALGO", raising=False)
    else:
        mp.setenv("RT_GPU_BVH_ALGO", builder)   # (read by rt_build_blas)
    c.set_param("blas_builder", 0 if builder == "host" else 1)


def to_device(inst):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(inst, INSTANCE_DTYPE).view(np.uint8).reshape(-1, 64).copy()).to("cuda:0")
    torch.cuda.current_stream().synchronize()
    return t


def set_inst(c, inst, path, update=False):
    if path == "host":
        c.set_instances(inst, update=update)
    else:
        c.set_instances_device(to_device(inst), update=update)


def instances_of(transforms, mesh):
    """rt_instance records: transforms (n, 12), mesh (n,) — object index = mesh, mask 0xFF"""
    out = np.repeat(np.array([host.make_instance(IDENTITY, 1, 0)], INSTANCE_DTYPE), len(mesh))
    out["transform"] = np.asarray(transforms, np.float32).reshape(-1, 12)
    out["mesh"] = mesh
    out["custom_index_and_mask"] = (0xFF << 24) | np.asarray(mesh, np.uint32)
    return out


@pytest.fixture(scope="module")
def ctx():
    c = RtContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def geom():
    return host.SceneGeometry(PATHS)


@pytest.mark.gpu
def test_snapshot_argument_checks(geom):
    c = RtContext(0)
    try:
        info = np.zeros(api.SNAPSHOT_INFO_WORDS, np.uint64)
        assert c.L.rt_debug_snapshot(c.h, 0, api._p(info), info.nbytes, None) == RT_ERR_NOT_READY          # no geometry, no TLAS
        c.upload_geometry(geom.verts, geom.idx, geom.ranges)
        assert c.L.rt_debug_snapshot(c.h, 0, api._p(info), info.nbytes, None) == RT_ERR_NOT_READY
        c.set_instances(host.SceneAnimation().instances((0, 1)))
        assert c.L.rt_debug_snapshot(c.h, 0, None, info.nbytes, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_debug_snapshot(c.h, 0, api._p(info), info.nbytes - 8, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_debug_snapshot(c.h, 9, api._p(info), info.nbytes, None) == RT_ERR_INVALID_ARGUMENT
        assert c.L.rt_debug_snapshot(c.h, 0, api._p(info), info.nbytes, None) == 0
        nodes = np.zeros(int(info[0]), api.NODEQ_DTYPE)
        assert c.L.rt_debug_snapshot(c.h, 1, api._p(nodes), nodes.nbytes - 32, None) == RT_ERR_INVALID_ARGUMENT   # short buffer
        snap = c.debug_snapshot()
        assert np.array_equal(snap["verts"], geom.verts) and np.array_equal(snap["idx"], geom.idx)
        assert snap["tlas_base"] >= snap["n_blas_nodes"] and snap["batch_k"] == 1 and len(snap["instances"]) == 2
        check(snap, [0, 1], [r[2] for r in geom.ranges])
        c.build_blas(1)                                                                                   # the TLAS is invalid again
        assert c.L.rt_debug_snapshot(c.h, 0, api._p(info), info.nbytes, None) == RT_ERR_NOT_READY
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("builder", BUILDERS)
def test_blas_producers_hold_the_contract(ctx, builder, monkeypatch):
    """every shape as a mesh of its own in one scene, one instance each, under the host builder and the three device builders; the
    records through rt_set_instances and through rt_set_instances_device"""
    use_builder(ctx, builder, monkeypatch)
    sh = cached_shapes()
    verts, idx, ranges = pack(list(sh.values()))
    ctx.upload_geometry(verts, idx, ranges)
    n = len(sh)
    inst = one_instance_each(n, shift=0.5)
    for path in ("host", "device"):
        set_inst(ctx, inst, path)
        snap = ctx.debug_snapshot()
        reached = check(snap, np.arange(n), [r[2] for r in ranges])
    print(builder, {name: reached["levels"][m] for m, name in enumerate(sh)})


def moved(geom, m, fn):
    """mesh m's vertex span (nv, 6) with its positions replaced by fn(positions), as a float32 tensor on the GPU"""
    import torch
    from tests.test_blas_refit import span
    ff, n = span(geom, m)
    v = geom.verts[ff:ff + n].reshape(-1, 6).copy()
    v[:, :3] = np.asarray(fn(v[:, :3].astype(np.float32)), np.float32)
    return torch.from_numpy(v).to("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["host", "3"])
def test_blas_refits_hold_the_contract(geom, builder, monkeypatch):
    """rt_refit_blas_device over trees of blas_builder 0 and 1: after every refit the slot that refitted AND a second frame slot of the
    scene re-issue their instances (update = 1) and are validated — boxes, packets, frontier boxes, the new q_lo / q_scale in every record"""
    import torch
    from tests.test_blas_refit import deform, span
    c = RtContext(0)
    try:
        use_builder(c, builder, monkeypatch)
        c.upload_geometry(geom.verts, geom.idx, geom.ranges)
        prims = [r[2] for r in geom.ranges]
        inst = host.SceneAnimation().instances((0, 1))
        c.set_instances(inst)
        slot = c.frame_slot()
        rng = np.random.default_rng(5)
        T = np.tile(IDENTITY, (3, 1))
        T[:, [3, 7, 11]] = rng.uniform(-6, 6, size=(3, 3))
        T[2, 0] = -1.5                                                          # mirrored
        inst2, mesh2 = instances_of(T, [1, 0, 0]), [1, 0, 0]
        slot.set_instances(inst2)
        check(c.debug_snapshot(), [0, 1], prims)
        check(slot.debug_snapshot(), mesh2, prims)
        current = {}

        def refit(m, t):
            torch.cuda.current_stream().synchronize()
            c.refit_blas_device(m, t)
            current[m] = t.cpu().numpy().reshape(-1)

        def validate_both(what, update=True):
            for who, s, i, im in (("refitting slot", c, inst, [0, 1]), ("second slot", slot, inst2, mesh2)):
                s.set_instances(i, update=update)
                snap = s.debug_snapshot()
                for m, t in current.items():                                     # the device vertex buffer is the truth after a refit
                    ff, n = span(geom, m)
                    assert np.array_equal(snap["verts"][ff:ff + n].view(np.uint32), t.view(np.uint32)), (what, who, m)
                viol, reached = tr.validate(snap, im)
                assert clean(viol) == {}, (what, who, clean(viol))
                assert reached["packets"] == dict(enumerate(prims)) and reached["instances"] == [len(im)], (what, who, reached)
            return snap

        q0 = c.debug_snapshot()["meshes"]["q_scale"][0].copy()
        refit(0, moved(geom, 0, lambda p: p))
        validate_both("identity")
        refit(0, deform(geom, 0))
        validate_both("sine deformation")
        refit(0, moved(geom, 0, lambda p: p * np.float32(100.0) + np.array([5000, -3000, 8000], np.float32)))
        snap = validate_both("scale by 100 and a far translation")
        assert (snap["meshes"]["q_scale"][0] > 50 * q0).all()                    # the dequantisation moved by orders of magnitude
        refit(0, moved(geom, 0, lambda p: p * np.array([1, 1, 0], np.float32)))
        snap = validate_both("collapse onto z = 0")
        assert snap["meshes"]["q_scale"][0][2] == np.float32(1e-30)
        refit(0, moved(geom, 0, lambda p: np.zeros_like(p) + np.array([0.3, -1.7, 2.9], np.float32)))
        snap = validate_both("collapse onto one point")
        assert (snap["meshes"]["q_scale"][0] == np.float32(1e-30)).all()
        for phase, amp in ((0.3, 0.2), (1.1, 0.05), (2.0, 0.3)):                 # back to back: arrival counters and scratch are reused
            refit(0, deform(geom, 0, amp=amp, phase=phase))
        validate_both("three refits back to back")
        refit(1, moved(geom, 1, lambda p: p * np.float32(0.37) + np.float32(0.11)))   # the two meshes share the scratch
        refit(0, deform(geom, 0, amp=0.1, phase=4.0, scale=(1.0, 2.5, 0.5)))
        validate_both("mesh 1, then mesh 0")
        refit(0, deform(geom, 0, amp=0.25, phase=5.0))
        c.build_blas(1)                                                           # relinks: the refit of mesh 0 is applied again from the device vertices
        validate_both("a refit, then rt_build_blas of the other mesh", update=False)
    finally:
        c.close()


# ---- TLAS ----

def _rot(rng):
    q = rng.normal(size=4); q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


FAMILIES = ["ring", "identical", "line", "mirror_shear", "scales", "far"]


def family(name, n, seed):
    """(n, 12) transforms of one family"""
    rng = np.random.default_rng(seed)
    T = np.zeros((n, 3, 4))
    if name == "ring":
        a = 2.0 * np.pi * (np.arange(n) + rng.uniform()) / n
        s = 0.12
        T[:, 0, 0], T[:, 0, 2], T[:, 1, 1], T[:, 2, 0], T[:, 2, 2] = s * np.cos(a), s * np.sin(a), s, -s * np.sin(a), s * np.cos(a)
        T[:, 0, 3], T[:, 1, 3], T[:, 2, 3] = 8.0 * np.cos(a), 0.9 * np.sin(7.0 * a), 8.0 * np.sin(a)
    elif name == "identical":                                                    # every Morton code is equal
        T[:] = np.concatenate([_rot(rng) * 0.4, rng.uniform(-3, 3, (3, 1))], axis=1)
    elif name == "line":                                                         # all centres on one line
        T[:, :, :3] = np.eye(3) * 0.05
        T[:, :, 3] = rng.uniform(-20, 20, (n, 1)) * np.array([1.0, 0.5, -2.0])
    elif name == "mirror_shear":
        for i in range(n):
            M = _rot(rng) @ np.diag(rng.uniform(0.05, 0.35, 3)) @ np.array([[1, rng.uniform(-0.6, 0.6), 0], [0, 1, rng.uniform(-0.6, 0.6)], [0, 0, 1]])
            T[i, :, :3] = M @ np.diag([-1.0 if i % 2 else 1.0, 1.0, 1.0])
        T[:, :, 3] = rng.uniform(-14, 14, (n, 3))
    elif name == "scales":                                                       # uniform scales from 1e-3 to 1e3
        T[:, :, :3] = np.eye(3) * (10.0 ** np.linspace(-3, 3, n) if n > 1 else np.array([1e3]))[rng.permutation(n), None, None]
        T[:, :, 3] = rng.uniform(-50, 50, (n, 3))
    elif name == "far":                                                          # one instance translated by 1e5
        T[:, :, :3] = np.eye(3) * 0.2
        T[:, :, 3] = rng.uniform(-10, 10, (n, 3))
        T[n // 2, 0, 3] += 1e5
    return T.reshape(n, 12).astype(np.float32)


def meshes_of(n):
    """teapot / cube alternating, every fifth instance names the empty mesh 2 (from three instances on)"""
    m = np.arange(n) % 2
    if n >= 3:
        m[2::5] = 2
    return m


@pytest.fixture(scope="module")
def tlas_ctx(geom):
    c = RtContext(0)
    verts, idx, ranges = geom.verts, geom.idx, list(geom.ranges) + [(0, len(geom.idx), 0)]   # mesh 2 has no triangles
    c.upload_geometry(verts, idx, ranges)
    yield c, [r[2] for r in ranges]
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["host", "device"])
@pytest.mark.parametrize("n", [1, 2, 3, 33, 1000, 4096])
def test_tlas_builds_and_refits_hold_the_contract(tlas_ctx, n, path):
    """the host TLAS (rt_set_instances) and the device TLAS (rt_set_instances_device), built and refitted: every family of transforms
    as a build, then a refit after every instance has moved far from where the topology was built (another family, other seed).
    Every kind but the depth is asserted per tree; the depth (<= 20 interior levels) is asserted last, over all families, so that a
    deep tree does not hide the other checks.

    The Karras radix tree of rt_set_instances_device is as deep as its keys make it: at n = 4096 it has 25 interior levels with all
    centres on one line, 22 mirrored and sheared, 21 with scales from 1e-3 to 1e3 (measured on an MI355X).  Such a build falls back to
    the balanced tree over the same Morton order (k_balanced_tree, ceil(log2 n) levels), which this case exercises, refits included."""
    c, prims = tlas_ctx
    mesh = meshes_of(n)
    want = int((np.asarray(prims)[mesh] > 0).sum())
    depth = {}
    for k, name in enumerate(FAMILIES):
        other = FAMILIES[(k + 2) % len(FAMILIES)]
        for what, fam, seed, update in ((name, name, 10 + k, False), (name + " refitted to " + other, other, 50 + k, True)):
            set_inst(c, instances_of(family(fam, n, seed=seed), mesh), path, update=update)
            viol, reached = tr.validate(c.debug_snapshot(), mesh)
            levels = reached["tlas_levels"][0]
            if viol.pop("tlas_depth"):
                assert levels > tr.TLAS_MAX_DEPTH
            assert clean(viol) == {}, (what, clean(viol))
            assert reached["packets"] == {m: pc for m, pc in enumerate(prims) if pc} and reached["instances"] == [want], (what, reached)
            depth[what] = levels
    print("TLAS interior levels, %s records, n = %d: %s" % (path, n, depth))
    assert max(depth.values()) <= tr.TLAS_MAX_DEPTH, depth


@pytest.mark.gpu
def test_frame_batch_trees_share_one_quantisation(tlas_ctx):
    """rt_set_batch with K = 8 frames of 33 instances with distinct transforms per frame, as a build and as an update: eight trees
    tlas_stride apart under one tlas_q_lo / tlas_q_scale, each naming its own frame's records"""
    c, prims = tlas_ctx
    K, n = 8, 33
    mesh = meshes_of(n)
    u = np.repeat(np.asarray(host.default_uniforms(max_bounce_count=1, samples_per_pixel=1, center_object_type=1, orbiting_object_type=0)).reshape(1), K)
    for update, seed in ((False, 100), (True, 200)):
        inst = np.stack([instances_of(family(FAMILIES[(f + (3 if update else 0)) % len(FAMILIES)], n, seed=seed + f), mesh) for f in range(K)])
        c.set_batch(inst, u, update=update)
        snap = c.debug_snapshot()
        assert snap["batch_k"] == K and snap["inst_per_frame"] == n and len(snap["instances"]) == K * n
        assert snap["tlas_stride"] >= snap["tlas_node_count"] and len(snap["tlas_nodes"]) == K * snap["tlas_stride"]
        check(snap, np.tile(mesh, K), prims, frames=K)
    c.set_instances(instances_of(family("ring", n, 1), mesh))                    # (back to a single frame for the tests that follow)


@pytest.mark.gpu
def test_two_frame_slots_hold_different_instance_sets(tlas_ctx):
    """two slots of one scene with different instance sets at the same time, host and device records: each slot's region is validated
    after the other slot's upload"""
    a, prims = tlas_ctx
    ma, mb = meshes_of(33), meshes_of(1000)
    a.set_instances(instances_of(family("ring", 33, 1), ma))
    b = a.frame_slot()
    try:
        for pa, pb in (("host", "device"), ("device", "host")):
            set_inst(a, instances_of(family("ring", 33, 2), ma), pa)
            set_inst(b, instances_of(family("mirror_shear", 1000, 3), mb), pb)
            sa, sb = a.debug_snapshot(), b.debug_snapshot()
            assert sa["tlas_base"] != sb["tlas_base"]
            check(sa, ma, prims)
            check(sb, mb, prims)
            set_inst(a, instances_of(family("far", 33, 4), ma), pa, update=True)
            check(b.debug_snapshot(), mb, prims)                                  # untouched by the other slot's refit
            set_inst(b, instances_of(family("scales", 1000, 5), mb), pb, update=True)
            check(a.debug_snapshot(), ma, prims)
            check(b.debug_snapshot(), mb, prims)
    finally:
        b.close()
