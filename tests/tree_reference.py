"""Node-by-node validator of the acceleration structures the kernels walk, in plain numpy and independent of the library's C++.

Input is a snapshot as RtContext.debug_snapshot returns it (or one assembled by hand, see link_meshes): the linked BLAS nodes, one
context's TLAS region, the triangle packets, the instance records, the device mesh table, the vertex and index buffers and the frontier
boxes.  `validate` visits every node, packet and instance once, level by level, and returns the number of violations per kind
("The contract of every tree producer").

Decisions are exact.  A plane is q_lo + q * q_scale in real arithmetic.  The difference between a coordinate and a plane is first
evaluated in binary64 together with a bound on its rounding error; whatever lies inside that bound (ties, axes with q_scale = 1e-30)
is decided with fractions.Fraction.  There is no tolerance anywhere."""
from fractions import Fraction

import numpy as np

BLAS_MAX_DEPTH = 40
TLAS_MAX_DEPTH = 20

KINDS = (
    # BLAS
    "blas_node_twice",       # a node slot reached twice (within a mesh or across meshes)
    "blas_link_range",       # an interior link outside [0, n_blas_nodes)
    "blas_inverted_link",    # a child with inverted planes whose link does not repeat its sibling's AND leads to an active triangle (a subtree
                             # of inactive triangles only keeps its link under inverted planes: a refit over good vertices revives it)
    "blas_leaf_range",       # a leaf whose packets do not lie inside the packet array
    "packet_twice",          # a packet reached more than once
    "packet_unreached",      # a mesh reaches fewer packets of active triangles than it has active triangles (an inactive one may be reached or not)
    "prim_permutation",      # the prim values of a mesh's packets are not a permutation of 0..prim_count-1
    "packet_bits",           # v0 / e1 / e2 differ from verts[idx[3p]], fl32(v1 - v0), fl32(v2 - v0)
    "blas_lo",               # a lower plane on the path lies above a vertex of the triangle
    "blas_hi",               # an upper plane on the path lies below a vertex of the triangle
    "frontier",              # a vertex of the mesh lies in none of its frontier boxes
    "blas_depth",            # interior levels differ from the mesh table's, or exceed BLAS_MAX_DEPTH
    # bad vertices (include/rt_api.h, rt_upload_geometry): a triangle with a position coordinate that is not finite or reaches 1e37 is INACTIVE
    "blas_not_finite",       # a q_lo or q_scale of a mesh (mesh table or record) that is not finite or not positive, or a last plane that is not finite
    "blas_bounds",           # the mesh table's lo / hi are not exactly the bounds of the mesh's ACTIVE triangles (none: lo > hi)
    "blas_frame",            # q_lo / q_scale are not bit for bit the documented function of those bounds (the host rule or the device rule)
    # TLAS
    "tlas_node_twice",
    "tlas_link_range",       # an interior link outside the frame's node range
    "tlas_inverted_link",
    "tlas_leaf_range",       # a leaf naming a record outside the frame's record range
    "instance_twice",
    "instance_unreached",    # an instance with triangles and a mask that is not 0 in no leaf
    "tlas_containment",      # a corner of the instance's transformed bounds outside the boxes on its path
    "record_fields",         # an InstanceDev field differs from the mesh table's current entry
    "tlas_depth",
    "void_record",           # a void record (void_records below) whose mask word is not 0, or whose leaf is drawn with another box than BOX_NONE
    "tlas_bounds",           # the TLAS dequantisation is not finite, or spans more than the records that are not void need
    "tlas_root_order",       # the root of a frame's TLAS has an absent (inverted) FIRST child beside a present second one: k_raygen and the ray
                             # generation of rt_shade_rays_device recognise the absent child of the root by its repeated link and take it to be child 1
)

_EPS = np.finfo(np.float64).eps


def cmp_plane(a, b, q_lo, q, s):
    """sign of (a + b) - (q_lo + q * s) in real arithmetic, elementwise (int8 array of -1, 0, 1).  a, b, q_lo and s are binary64 arrays
    (holding binary32 values, or binary64 ones), q integers in 0..65535."""
    a, b, q_lo, q, s = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(q_lo, np.float64),
                                           np.asarray(q, np.float64), np.asarray(s, np.float64))
    shape = a.shape
    a, b, q_lo, q, s = (x.reshape(-1) for x in (a, b, q_lo, q, s))
    qs = q * s                                      # (its rounding, if any, is inside the bound below)
    d = (a + b) - (q_lo + qs)
    bound = 16.0 * _EPS * (np.abs(a) + np.abs(b) + np.abs(q_lo) + np.abs(qs))
    out = np.sign(d).astype(np.int8)
    tie = ~(np.abs(d) > bound)
    if tie.any():
        rows = np.stack([a[tie], b[tie], q_lo[tie], q[tie], s[tie]], axis=1)
        uniq, inv = np.unique(rows, axis=0, return_inverse=True)
        res = np.empty(len(uniq), np.int8)
        for i, (ua, ub, ul, uq, us) in enumerate(uniq.tolist()):
            e = Fraction(ua) + Fraction(ub) - Fraction(ul) - int(uq) * Fraction(us)
            res[i] = (e > 0) - (e < 0)
        out[tie] = res[np.asarray(inv).reshape(-1)]
    return out.reshape(shape)


def _walk(nodes, first_global, root, lo_ok, hi_ok, visited, out, prefix, max_iter, follow_absent=False):
    """Level-by-level walk of one tree.  nodes[i] is global node first_global + i; links must stay inside [lo_ok, hi_ok); visited is the
    shared per-slot flag array of `nodes`.  Every entered child carries the intersection (in quanta) of the child boxes on its path.
    follow_absent (a BLAS): a child with inverted planes and a link of its own is entered all the same, as ABSENT — what lies below it
    is in no box; the caller decides whether that is a violation (an active triangle there) — and is not counted as an inverted link here.
    Returns (leaf refs, leaf lo (n, 3), leaf hi (n, 3), interior levels, nodes visited, shape_ok, leaf absent (n,) bool)."""
    bad0 = out[prefix + "_node_twice"] + out[prefix + "_link_range"] + out[prefix + "_inverted_link"]
    cur = np.array([root], np.int64)
    blo = np.zeros((1, 3), np.int64)
    bhi = np.full((1, 3), 65535, np.int64)
    dead = np.zeros(1, bool)
    leaves, llo, lhi, ldead = [], [], [], []
    levels = n_visited = 0
    for _ in range(max_iter):
        ok = (cur >= lo_ok) & (cur < hi_ok)
        out[prefix + "_link_range"] += int((~ok).sum())
        cur, blo, bhi, dead = cur[ok], blo[ok], bhi[ok], dead[ok]
        loc = cur - first_global
        _, first_at = np.unique(loc, return_index=True)
        fresh = np.zeros(len(loc), bool)
        fresh[first_at] = True
        fresh &= ~visited[loc]
        out[prefix + "_node_twice"] += int((~fresh).sum())
        cur, blo, bhi, loc, dead = cur[fresh], blo[fresh], bhi[fresh], loc[fresh], dead[fresh]
        if not len(cur):
            break
        visited[loc] = True
        levels += 1
        n_visited += len(cur)
        w = nodes["w"][loc].astype(np.int64).reshape(-1, 2, 3)
        ch = nodes["child"][loc].astype(np.int64)
        qlo, qhi = w & 0xFFFF, w >> 16
        inverted = (qlo > qhi).any(axis=2)                                  # (n, 2)
        own = inverted & (ch != ch[:, ::-1])
        if not follow_absent:
            out[prefix + "_inverted_link"] += int(own.sum())
        nlo = np.maximum(blo[:, None, :], qlo)
        nhi = np.minimum(bhi[:, None, :], qhi)
        enter = ~inverted | (own if follow_absent else False)
        ndead = (dead[:, None] | inverted)[enter]
        ref, nlo, nhi = ch[enter], nlo[enter], nhi[enter]
        leaf = ref < 0
        leaves.append(~ref[leaf]); llo.append(nlo[leaf]); lhi.append(nhi[leaf]); ldead.append(ndead[leaf])
        cur, blo, bhi, dead = ref[~leaf], nlo[~leaf], nhi[~leaf], ndead[~leaf]
    else:
        out[prefix + "_node_twice"] += 1                                    # (cannot happen: every slot is entered once)
    shape_ok = out[prefix + "_node_twice"] + out[prefix + "_link_range"] + out[prefix + "_inverted_link"] == bad0
    cat = lambda xs, shape: np.concatenate(xs) if xs else np.zeros(shape, np.int64)
    return cat(leaves, (0,)), cat(llo, (0, 3)), cat(lhi, (0, 3)), levels, n_visited, shape_ok, (np.concatenate(ldead) if ldead else np.zeros(0, bool))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


INST_BOX_LIMIT = np.float32(1e37)


def padded_world_box(o2w, lo, hi):
    """instance_world_box (csrc/rt_api.cpp, k_inst_records) in numpy: the eight corners of the mesh bounds through o2w in binary64,
    rounded to binary32, min / max that drop a NaN, padded by 1e-5 of the largest magnitude + 1e-30 in binary32.  o2w (n, 12), lo and
    hi (n, 3) -> (lo, hi) float32 (n, 3)"""
    f = np.float32
    M = np.asarray(o2w, f).astype(np.float64).reshape(-1, 3, 4)
    corner = np.array([[(c >> a) & 1 for a in range(3)] for c in range(8)], bool)
    p = np.where(corner[None], np.asarray(hi, f).astype(np.float64)[:, None, :], np.asarray(lo, f).astype(np.float64)[:, None, :])   # (n, 8, 3)
    with np.errstate(all="ignore"):
        v = ((M[:, None, :, 0] * p[:, :, None, 0] + M[:, None, :, 1] * p[:, :, None, 1]) + M[:, None, :, 2] * p[:, :, None, 2]) + M[:, None, :, 3]
        v32 = v.astype(f)                                                                     # (n, 8, 3)
        wlo = np.fmin(f(3.0e38), np.fmin.reduce(v32, axis=1))
        whi = np.fmax(f(-3.0e38), np.fmax.reduce(v32, axis=1))
        mag = np.fmax(f(0), np.fmax.reduce(np.abs(v).astype(f).reshape(len(M), -1), axis=1))
        pad = (f(1e-5) * mag + f(1e-30)).astype(f)
        return (wlo - pad[:, None]).astype(f), (whi + pad[:, None]).astype(f)


BAD_COORD_LIMIT = INST_BOX_LIMIT


def active_triangles(P):
    """P (n, 3 corners, 3 axes) float32 -> (n,) bool: every one of the nine coordinates finite and of magnitude below BAD_COORD_LIMIT
    (include/rt_api.h, rt_upload_geometry: the others are BAD triangles, inactive in every builder and consumer)"""
    with np.errstate(invalid="ignore"):
        return (np.abs(np.asarray(P, np.float32)) < BAD_COORD_LIMIT).reshape(len(P), -1).all(axis=1)


def active_bounds(P):
    """(lo, hi) float32 over the vertices of the active triangles of P; none: the empty box (3e38, -3e38)"""
    A = np.asarray(P, np.float32)[active_triangles(P)].reshape(-1, 3)
    if not len(A):
        return np.full(3, 3.0e38, np.float32), np.full(3, -3.0e38, np.float32)
    return A.min(axis=0), A.max(axis=0)


def frame_rules(lo, hi):
    """the two documented dequantisations of a mesh with bounds [lo, hi] (an empty box counts as [0, 0]), as (q_lo, q_scale) float32
    pairs: the host's (quant_params of csrc/bvh_build.cpp: 65530 quanta of the extent times 1 + 1e-6 in binary64, two quanta below) and
    the device builders' and the refit's (csrc/blas_quant.h: 65520 quanta of the extent times 1.00001 in binary32, four quanta below)"""
    f = np.float32
    lo, hi = np.asarray(lo, f), np.asarray(hi, f)
    if (lo > hi).any():
        lo = hi = np.zeros(3, f)
    ext = (hi - lo).astype(f)
    scale = np.where(ext > 0, ((ext * f(1.00001)).astype(f) / f(65520.0)).astype(f), f(1e-30)).astype(f)
    return quant_params(lo, hi), ((lo - (f(4.0) * scale).astype(f)).astype(f), scale)


def void_records(inst, meshes, inst_mesh):
    """(n,) bool: the records of meshes with triangles that the contract calls void (include/rt_api.h, rt_set_instances): an entry of
    the transform that is not finite, or a padded world box with a coordinate of magnitude 1e37 or more"""
    mt = meshes[np.asarray(inst_mesh, np.int64)]
    o2w = np.asarray(inst["o2w"], np.float32).reshape(-1, 12)
    lo, hi = padded_world_box(o2w, mt["lo"], mt["hi"])
    with np.errstate(invalid="ignore"):
        inside = (np.abs(lo) < INST_BOX_LIMIT).all(axis=1) & (np.abs(hi) < INST_BOX_LIMIT).all(axis=1)
    return (mt["prim_count"] > 0) & ~(np.isfinite(o2w).all(axis=1) & inside)


def validate(snap, inst_mesh, blas=True):
    """snap: a snapshot (RtContext.debug_snapshot / link_meshes); inst_mesh: the mesh index of every instance record (all frames of a
    batch).  Returns (violations, reached): violations maps every kind of KINDS to a count; reached holds what the walk visited —
    packets[m], nodes[m], leaves[m], levels[m] per mesh with triangles, instances[k] and tlas_levels[k] per frame.  blas=False checks the
    records and the TLAS only (for a snapshot whose meshes an earlier call has validated: a new set of instances leaves them alone)."""
    out = {k: 0 for k in KINDS}
    reached = {"packets": {}, "active": {}, "inactive": {}, "nodes": {}, "leaves": {}, "levels": {}, "instances": [], "tlas_levels": []}
    meshes, inst, packets = snap["meshes"], snap["instances"], snap["packets"]
    inst_mesh = np.asarray(inst_mesh, np.int64)
    assert len(inst_mesh) == len(inst)
    verts, idx = snap["verts"], snap["idx"]
    bn = snap["blas_nodes"]
    n_blas, n_pk = len(bn), len(packets)

    # ---- record fields: every InstanceDev carries the mesh table's current entry, bit for bit ----
    mt = meshes[inst_mesh]
    for f in ("blas_root", "first_float", "first_index", "cover_first", "cover_count"):
        out["record_fields"] += int((inst[f] != mt[f]).sum())
    for f in ("q_lo", "q_scale"):
        out["record_fields"] += int((_bits(inst[f]) != _bits(mt[f])).sum())

    # ---- BLAS ----
    visited = np.zeros(n_blas, bool)
    pk_count = np.zeros(n_pk, np.int64)
    mesh_bounds = {}
    for m in range(len(meshes)):
        M = meshes[m]
        pc = int(M["prim_count"])
        if pc == 0:
            continue
        users = np.nonzero(inst_mesh == m)[0]
        src = inst[users[0]] if len(users) else M                            # the dequantisation the kernels use
        q_lo, q_s = src["q_lo"].astype(np.float64), src["q_scale"].astype(np.float64)
        ff, fi = int(M["first_float"]), int(M["first_index"])
        tri = idx[fi:fi + 3 * pc].astype(np.int64).reshape(-1, 3)
        pos = verts[ff:].reshape(-1)                                         # position of vertex v: pos[6v : 6v + 3]
        P = np.stack([pos[6 * tri + a] for a in range(3)], axis=2)           # (pc, 3 corners, 3 axes) float32
        active = active_triangles(P)
        used = np.unique(tri[active])
        vp = np.stack([pos[6 * used + a] for a in range(3)], axis=1)         # positions the active triangles reference
        mesh_bounds[m] = active_bounds(P)
        if not blas:
            continue

        # ---- the frame: finite, and exactly that of the active triangles ----
        not_finite = 0
        with np.errstate(all="ignore"):
            for src_ in ([M] + [inst[u] for u in users]):
                fl, fs = src_["q_lo"].astype(np.float64), src_["q_scale"].astype(np.float64)
                not_finite += int((~(np.isfinite(fl) & np.isfinite(fs) & (fs > 0) & np.isfinite((fl + 65535.0 * fs).astype(np.float32)))).sum())
        out["blas_not_finite"] += not_finite
        if not_finite:
            continue                                                         # (no plane of this mesh is a number: nothing below can be decided)
        # (as numbers: all of them are finite or the empty box's 3e38, and a minimum over -0 and +0 has either sign)
        out["blas_bounds"] += int((M["lo"] != mesh_bounds[m][0]).sum() + (M["hi"] != mesh_bounds[m][1]).sum())
        rules = frame_rules(*mesh_bounds[m])
        if not any((_bits(M["q_lo"]) == _bits(r[0])).all() and (_bits(M["q_scale"]) == _bits(r[1])).all() for r in rules):
            out["blas_frame"] += 1

        refs, llo, lhi, levels, n_nodes, shape_ok, ldead = _walk(bn, 0, int(M["blas_root"]), 0, n_blas, visited, out, "blas", n_blas + 2, follow_absent=True)
        first, cnt = refs >> 3, (refs & 7) + 1
        in_range = first + cnt <= n_pk
        out["blas_leaf_range"] += int((~in_range).sum())
        first, cnt, llo, lhi, ldead = first[in_range], cnt[in_range], llo[in_range], lhi[in_range], ldead[in_range]
        leaf_of = np.repeat(np.arange(len(first)), cnt)
        pk = np.repeat(first, cnt) + (np.arange(len(leaf_of)) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        upk, ucnt = np.unique(pk, return_counts=True)
        out["packet_twice"] += int(((ucnt > 1) | (pk_count[upk] > 0)).sum())      # within this mesh, or already reached from another
        pk_count[upk] += ucnt
        reached["packets"][m], reached["nodes"][m], reached["leaves"][m], reached["levels"][m] = len(upk), n_nodes, len(refs), levels
        uprim = packets["prim"][upk].astype(np.int64)
        n_active_reached = int(active[uprim[uprim < pc]].sum())
        reached["active"][m], reached["inactive"][m] = n_active_reached, int(pc - active.sum())
        if shape_ok:
            out["packet_unreached"] += max(0, int(active.sum()) - n_active_reached)
            if levels != int(M["levels"]) or levels > BLAS_MAX_DEPTH:
                out["blas_depth"] += 1
        prim = packets["prim"][upk].astype(np.int64)
        good = prim < pc
        out["prim_permutation"] += int((~good).sum()) + int(len(prim[good]) - len(np.unique(prim[good])))

        # packets against the vertex and index buffers, bit for bit
        prim_all = packets["prim"][pk].astype(np.int64)
        okp = prim_all < pc
        pk, leaf_of, prim_all = pk[okp], leaf_of[okp], prim_all[okp]
        T = P[prim_all]                                                      # (n, 3, 3)
        rec = packets[pk]
        with np.errstate(all="ignore"):                                      # (a NaN edge of an inactive triangle is a NaN: its payload is the processor's)
            differs = lambda got, want: ((_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want))).any(axis=1)
            bad = differs(rec["v0"], T[:, 0]) | differs(rec["e1"], T[:, 1] - T[:, 0]) | differs(rec["e2"], T[:, 2] - T[:, 0])
        out["packet_bits"] += int(bad.sum())
        # an inverted child that keeps a link of its own may hold inactive triangles only
        act = active[prim_all]
        out["blas_inverted_link"] += int(np.unique(leaf_of[act & ldead[leaf_of]]).size)
        act &= ~ldead[leaf_of]                                               # containment: the active triangles (those below an absent child are counted above)
        pk, leaf_of, T, rec = pk[act], leaf_of[act], T[act], rec[act]

        # containment along the path: the three buffer positions, and the exact v0, v0 + e1, v0 + e2 of the packet
        v0 = rec["v0"].astype(np.float64)
        a = np.concatenate([T.astype(np.float64), np.stack([v0, v0, v0], axis=1)], axis=1)                        # (n, 6, 3)
        b = np.concatenate([np.zeros_like(T, dtype=np.float64),
                            np.stack([np.zeros_like(v0), rec["e1"].astype(np.float64), rec["e2"].astype(np.float64)], axis=1)], axis=1)
        lo_q, hi_q = llo[leaf_of][:, None, :], lhi[leaf_of][:, None, :]
        out["blas_lo"] += int((cmp_plane(a, b, q_lo, lo_q, q_s) < 0).sum())
        out["blas_hi"] += int((cmp_plane(a, b, q_lo, hi_q, q_s) > 0).sum())

        # frontier boxes: every referenced position in at least one
        cf, cc = int(M["cover_first"]), int(M["cover_count"])
        boxes = snap["cover_boxes"][cf:cf + cc]
        covered = np.zeros(len(vp), bool)
        for s0 in range(0, len(vp), 2048):
            v = vp[s0:s0 + 2048][:, None, :]
            covered[s0:s0 + 2048] = ((v >= boxes[None, :, :3]) & (v <= boxes[None, :, 3:])).all(axis=2).any(axis=1)
        out["frontier"] += int((~covered).sum())

    # ---- TLAS ----
    tn = snap["tlas_nodes"]
    K, n = int(snap["batch_k"]), int(snap["inst_per_frame"])
    base, count = int(snap["tlas_base"]), int(snap["tlas_node_count"])
    stride = int(snap["tlas_stride"]) if K > 1 else 0
    t_lo, t_s = np.asarray(snap["tlas_q_lo"], np.float32).astype(np.float64), np.asarray(snap["tlas_q_scale"], np.float32).astype(np.float64)
    tvisited = np.zeros(len(tn), bool)
    has_tris = meshes["prim_count"][inst_mesh] > 0
    # ---- void records: mask word 0, nothing of them in the bounds ----
    void = void_records(inst, meshes, inst_mesh)
    out["void_record"] += int((void & (inst["mask"] != 0)).sum())
    out["tlas_bounds"] += _bounds_excess(inst, meshes, inst_mesh, has_tris & ~void, t_lo, t_s)
    for k in range(K):
        root = base + k * stride
        if 0 <= root - base < len(tn):
            rw = tn["w"][root - base].astype(np.int64).reshape(2, 3)
            absent = ((rw & 0xFFFF) > (rw >> 16)).any(axis=1)
            out["tlas_root_order"] += int(absent[0] and not absent[1])
        refs, llo, lhi, levels, _, shape_ok, _ = _walk(tn, base, root, root, root + count, tvisited, out, "tlas", len(tn) + 2)
        in_frame = (refs >= k * n) & (refs < (k + 1) * n)
        out["tlas_leaf_range"] += int((~in_frame).sum())
        refs, llo, lhi = refs[in_frame], llo[in_frame], lhi[in_frame]
        times = np.bincount(refs - k * n, minlength=n)
        out["instance_twice"] += int((times > 1).sum())
        need = has_tris[k * n:(k + 1) * n] & (inst["mask"][k * n:(k + 1) * n] != 0) & ~void[k * n:(k + 1) * n]   # (a void record: "void_record")
        if shape_ok:
            out["instance_unreached"] += int((need & (times == 0)).sum())
            if levels > TLAS_MAX_DEPTH:
                out["tlas_depth"] += 1
        reached["instances"].append(int((has_tris[k * n:(k + 1) * n] & (times > 0)).sum()))
        reached["tlas_levels"].append(levels)
        out["void_record"] += int((void[refs] & (llo != 65535).any(axis=1)).sum())                  # (BOX_NONE lies above every plane)
        sel = has_tris[refs] & ~void[refs]
        refs, llo, lhi = refs[sel], llo[sel], lhi[sel]
        if not len(refs):
            continue
        lo = np.stack([mesh_bounds[int(m)][0] for m in inst_mesh[refs]]).astype(np.float64)
        hi = np.stack([mesh_bounds[int(m)][1] for m in inst_mesh[refs]]).astype(np.float64)
        corner = np.array([[(c >> a) & 1 for a in range(3)] for c in range(8)], bool)                 # (8, 3)
        p = np.where(corner[None], hi[:, None, :], lo[:, None, :])                                    # (r, 8, 3)
        o2w = inst["o2w"][refs].astype(np.float64).reshape(-1, 3, 4)
        img = (o2w[:, None, :, 0] * p[:, :, None, 0] + o2w[:, None, :, 1] * p[:, :, None, 1] + o2w[:, None, :, 2] * p[:, :, None, 2]) + o2w[:, None, :, 3]
        out["tlas_containment"] += int((cmp_plane(img, 0.0, t_lo, llo[:, None, :], t_s) < 0).sum())
        out["tlas_containment"] += int((cmp_plane(img, 0.0, t_lo, lhi[:, None, :], t_s) > 0).sum())
    return out, reached


def _bounds_excess(inst, meshes, inst_mesh, valid, t_lo, t_s):
    """The number of axes on which the dequantisation (t_lo, t_s) is not finite or spans more than the `valid` records need by the
    documented rule.  With [L, H] the union of their world boxes, each padded by at most 1.01e-5 of its largest magnitude + 2e-30:
    q_scale <= s = (H - L)(1 + 1e-6) / 65530 (1e-30 for H = L), q_lo = lo - 2 q_scale >= L - 2 s and the last plane q_lo + 65535
    q_scale = lo + 65533 q_scale <= (their smallest lo) + 65533 s, each up to the binary32 rounding of the two numbers (below 1e-6 (|L| + |H|)).  A box
    that is not one of theirs and reaches the bounds (a void record's, an empty mesh's 3e38) breaks this by orders of magnitude."""
    t_lo, t_s = np.asarray(t_lo, np.float64), np.asarray(t_s, np.float64)
    bad = ~(np.isfinite(t_lo) & np.isfinite(t_s) & (t_s > 0))
    if valid.any():
        mt = meshes[np.asarray(inst_mesh, np.int64)[valid]]
        lo, hi = padded_world_box(np.asarray(inst["o2w"], np.float32).reshape(-1, 12)[valid], mt["lo"], mt["hi"])
        lo, hi = lo.astype(np.float64), hi.astype(np.float64)
        grow = 1e-7 * np.maximum(np.abs(lo), np.abs(hi)).max(axis=1, keepdims=True) + 1e-30          # (the pad itself is inside lo / hi)
        L, H, first = (lo - grow).min(axis=0), (hi + grow).max(axis=0), lo.min(axis=0)
    else:
        L = H = first = np.zeros(3)
    s = np.maximum((H - L) * (1.0 + 1e-6) / 65530.0, 1e-30)
    slack = 1e-6 * (np.abs(L) + np.abs(H)) + 1e-29
    with np.errstate(all="ignore"):
        top = t_lo + 65535.0 * t_s
        bad |= ~(t_lo >= L - 3.0 * s - slack) | ~(top <= first + 65534.0 * s + slack)
    return int(bad.sum())


# ---- snapshots assembled by hand (the self-test of the validator, host-built trees without a GPU) --------------------------------------

def quantise_box(lo, hi, q_lo, q_scale, margin):
    """the documented rule: lower planes rounded down and upper planes rounded up, `margin` whole quanta further out, clamped to 16 bits.
    lo, hi (3,) floats; returns the three words lo | hi << 16."""
    base, scale = np.asarray(q_lo, np.float32).astype(np.float64), np.asarray(q_scale, np.float32).astype(np.float64)
    ql = np.clip(np.floor((np.asarray(lo, np.float64) - base) / scale) - margin, 0, 65535).astype(np.int64)
    qh = np.clip(np.ceil((np.asarray(hi, np.float64) - base) / scale) + margin, 0, 65535).astype(np.int64)
    return (ql | (qh << 16)).astype(np.uint32)


def quant_params(lo, hi, quanta=65530.0, below=2.0):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    ext = hi - lo
    scale = np.where(ext > 0, ext * (1.0 + 1e-6) / quanta, 1e-30)
    return (lo - below * scale).astype(np.float32), scale.astype(np.float32)


INVERTED = np.uint32(0x0000FFFF)


def world_box(o2w, lo, hi):
    corner = np.array([[(c >> a) & 1 for a in range(3)] for c in range(8)], bool)
    p = np.where(corner, np.asarray(hi, np.float64), np.asarray(lo, np.float64))
    M = np.asarray(o2w, np.float64).reshape(3, 4)
    img = p @ M[:, :3].T + M[:, 3]
    return img.min(axis=0), img.max(axis=0)


def build_tree(topo, leaf_box, leaf_ref, q_lo, q_scale, margin=1, first=0, keep_links=False):
    """BvhNodeQ records of the tree `topo`: an interior node is a tuple of one or two children, anything else is a leaf.  leaf_box(leaf)
    gives (lo, hi) or None for a leaf without a box (its planes are inverted and its link repeats the sibling's, as quantize_bvh2_in
    leaves it); leaf_ref(leaf) the value a leaf link names.  Interior links are first + index.  A root that is a leaf gets the synthetic
    single-child root.  keep_links: a child without a box keeps its own link under the inverted planes (a BLAS child over inactive
    triangles only, as quantize_bvh2 with keep_links and the device builders leave it)."""
    from vulkan_raytracing_amd.api import NODEQ_DTYPE
    if not isinstance(topo, tuple):
        topo = (topo,)
    recs = []

    def box_of(t):
        if not isinstance(t, tuple):
            return leaf_box(t)
        bs = [b for b in (box_of(c) for c in t) if b is not None]
        return (np.min([b[0] for b in bs], axis=0), np.max([b[1] for b in bs], axis=0)) if bs else None

    def emit(t):
        i = len(recs)
        recs.append(None)
        w, link = np.full(6, INVERTED, np.uint32), [None, None]
        for k, c in enumerate(t):
            b = box_of(c)
            if b is not None:
                w[3 * k:3 * k + 3] = quantise_box(b[0], b[1], q_lo, q_scale, margin)
            if b is not None or keep_links:
                link[k] = first + emit(c) if isinstance(c, tuple) else ~int(leaf_ref(c))
        if link[0] is None:
            link[0] = link[1]
        if link[1] is None:
            link[1] = link[0]
        recs[i] = (w, link)
        return i

    emit(topo)
    out = np.zeros(len(recs), NODEQ_DTYPE)
    for i, (w, link) in enumerate(recs):
        out[i]["w"] = w
        out[i]["child"] = link
    return out


def balanced(items):
    items = list(items)
    if len(items) == 1:
        return items[0]
    h = len(items) // 2
    return (balanced(items[:h]), balanced(items[h:]))


def link_meshes(parts, transforms=None):
    """A snapshot of host-built meshes without a GPU.  parts: one (verts6, idx, nodes, packets, q_lo, q_scale, levels) per mesh, nodes
    and packets as rt_debug_host_blas returns them (links local to the mesh).  One instance per mesh (identity unless given), a TLAS
    quantised by the documented rule, one frontier box per mesh (its bounds).  Returns (snapshot, mesh index of every instance)."""
    from vulkan_raytracing_amd.api import INSTANCE_DEV_DTYPE, NODEQ_DTYPE, TLAS_MESH_DTYPE, TRI_PACKET_DTYPE
    n = len(parts)
    meshes, inst = np.zeros(n, TLAS_MESH_DTYPE), np.zeros(n, INSTANCE_DEV_DTYPE)
    nodes, packets, verts, idx, cover = [], [], [], [], []
    nn = nt = nf = ni = 0
    for m, (v, ix, nd, pk, q_lo, q_scale, levels) in enumerate(parts):
        v, ix = np.ascontiguousarray(v, np.float32).reshape(-1), np.ascontiguousarray(ix, np.uint32).reshape(-1)
        nd = nd.copy()
        ch = nd["child"].astype(np.int64)
        ref = ~ch
        nd["child"] = np.where(ch >= 0, ch + nn, ~((((ref >> 3) + nt) << 3) | (ref & 7))).astype(np.int32)
        lo, hi = active_bounds(v.reshape(-1, 6)[ix.astype(np.int64), :3].reshape(-1, 3, 3))
        meshes[m] = (nn, 0, nf, ni, m, 1, len(ix) // 3, 1, levels, q_lo, q_scale, lo, hi)
        M = np.eye(4, dtype=np.float32)[:3].reshape(12) if transforms is None else np.asarray(transforms[m], np.float32).reshape(12)
        inst[m]["o2w"] = M
        inst[m]["w2o"] = np.linalg.inv(np.vstack([M.reshape(3, 4).astype(np.float64), [0, 0, 0, 1]]))[:3].reshape(12).astype(np.float32)
        for f in ("blas_root", "first_float", "first_index", "cover_first", "cover_count", "q_lo", "q_scale"):
            inst[m][f] = meshes[m][f]
        with np.errstate(all="ignore"):                                          # (every triangle inactive, or bounds that reach the instance limit: a void record)
            plo, phi = padded_world_box(M[None], lo[None], hi[None])
            inst[m]["mask"] = 0xFF if ((np.abs(plo) < INST_BOX_LIMIT).all() and (np.abs(phi) < INST_BOX_LIMIT).all()) else 0
        cover.append(np.concatenate([lo, hi]))
        nodes.append(nd); packets.append(pk); verts.append(v); idx.append(ix)
        nn += len(nd); nt += len(pk); nf += len(v); ni += len(ix)
    boxes = [world_box(inst[m]["o2w"], meshes[m]["lo"], meshes[m]["hi"]) if inst[m]["mask"] else None for m in range(n)]
    some = [b for b in boxes if b is not None] or [(np.zeros(3), np.zeros(3))]
    t_lo, t_s = quant_params(np.min([b[0] for b in some], axis=0), np.max([b[1] for b in some], axis=0))
    base = nn + 8
    tlas = build_tree(balanced(range(n)), lambda i: boxes[i], lambda i: i, t_lo, t_s, margin=1, first=base)
    snap = {"n_blas_nodes": nn, "tlas_base": base, "tlas_node_count": len(tlas), "tlas_stride": 0, "batch_k": 1, "inst_per_frame": n,
            "tlas_q_lo": t_lo, "tlas_q_scale": t_s, "blas_nodes": np.concatenate(nodes).astype(NODEQ_DTYPE), "tlas_nodes": tlas,
            "packets": np.concatenate(packets).astype(TRI_PACKET_DTYPE), "instances": inst, "meshes": meshes,
            "verts": np.concatenate(verts), "idx": np.concatenate(idx), "cover_boxes": np.array(cover, np.float32).reshape(-1, 6)}
    return snap, np.arange(n)
