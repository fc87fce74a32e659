// kernels_overlap.inc — included by kernels.hip after kernels_closest.inc (product and alt translation units alike).
// rt_overlap_boxes_device: for every query box the triangles of the scene that touch it — their number and the smallest of them by
// (inst, prim).  A record-level walk of its own (walk_common.inc: the stack, the chunk feed, the trip exit, the counters), one lane per
// box: no frame kernel and no existing query kernel changes.
//
//  * the node test is box against box on the dequantised planes, the query box inflated (DESIGN.md §5 "Box overlaps"): in world space by
//    2^-13 of the magnitudes that enter a candidate's world vertices (the box, the TLAS bounds, the row terms of every o2w: word 0 of
//    k_closest_scale's array); inside an instance the query is the bound of that inflated box's eight corners under w2o, inflated again
//    by 2^-13 of the mesh's bounds and of the row terms of w2o over the corners.  An instance with s_i == 0 (singular or non-finite
//    transform) or a non-finite bound gets an unbounded query: it does not prune.  Comparisons are written so that a NaN opens the node;
//  * the triangle test is the canonical sequence of DESIGN.md §5 in world space (overlap_tri): it depends on the box, the instance
//    record and the packet only, so the candidate set is the same whatever the tree;
//  * the list: in the lane's own row of the caller's id array, kept sorted by (inst, prim) by insertion; only the count and the row's
//    last entry live in registers, as in k_query_hits;
//  * pruning (no counts wanted): once the row is full, instances above the last entry's are not entered and triangles that do not
//    precede it are not tested; RT_OVERLAP_ANY ends the box at its first candidate.
#ifndef RT_OVERLAP_WAVES_PER_EU
#define RT_OVERLAP_WAVES_PER_EU 4   /* the record-level walks' budget */
#endif

struct IdRec { int32_t inst, prim; };   // 8 bytes, 4-byte aligned like the caller's rows

struct OverlapArgs {
  SceneDev sc;
  const float4* boxes;         // n records of 32 bytes: (lo.xyz, w3), (hi.xyz, w7)
  const float* inst_scale;     // k_closest_scale: [0] the largest row-term magnitude of any instance's o2w, [1 + i] s_i
  uint32_t cull_mask;
  uint32_t n;
  uint32_t k;                  // max_ids: 0..16 entries per row
  uint32_t any;                // RT_OVERLAP_ANY: the count is 0 or 1, the box ends at its first candidate
  IdRec* ids;                  // n * k records (inst, prim) (k == 0: null)
  uint32_t* counts;            // n counts, or null (then the walk prunes)
  uint32_t* cursor;            // chunk cursor (zero before the launch)
  uint32_t* counters;          // the query's counter block (counting form: CNT_NODE_VISITS, CNT_TRI_TESTS)
  int32_t* ovf_stack;          // ovf_stride ints per thread of the grid
  // the LIST instantiations only (kernels_list.inc); behind everything else, so that the other kernels read their arguments where they did
  const unsigned long long* offsets;   // n + 1 row starts: row i is ids[offsets[i] .. offsets[i + 1])
  unsigned long long capacity; // records of ids: a row that ends beyond it is not written
  uint32_t* worklist;          // the rows left in walk order (longer than RT_LIST_INSERT_MAX), for k_list_sort
  uint32_t* work_count;        // their number (zero before the launch)
};

constexpr float OB_ABS = 1.220703125e-04f;          // 2^-13: absolute slack per unit of magnitude

// the smallest projection beyond the radius or the largest below its negative (strict: a tie is not a separation; fminf / fmaxf:
// a NaN among numbers is passed over, three NaNs separate nothing).  The predicate is evaluated without branches, every axis of it.
__device__ __forceinline__ bool axis_separates(float p0, float p1, float p2, float r) {
  const bool above = fminf(fminf(p0, p1), p2) > r, below = fmaxf(fmaxf(p0, p1), p2) < -r;
  return above | below;
}
// the three axes e_x x f, e_y x f, e_z x f of one edge f against the centred triangle (v0, v1, v2) and the half extent h
__device__ __forceinline__ bool edge_separates(F3 f, F3 v0, F3 v1, F3 v2, F3 h) {
  const F3 af = mk3(__builtin_fabsf(f.x), __builtin_fabsf(f.y), __builtin_fabsf(f.z));
  const bool sx = axis_separates(v0.z * f.y - v0.y * f.z, v1.z * f.y - v1.y * f.z, v2.z * f.y - v2.y * f.z, h.y * af.z + h.z * af.y);
  const bool sy = axis_separates(v0.x * f.z - v0.z * f.x, v1.x * f.z - v1.z * f.x, v2.x * f.z - v2.z * f.x, h.x * af.z + h.z * af.x);
  const bool sz = axis_separates(v0.y * f.x - v0.x * f.y, v1.y * f.x - v1.x * f.y, v2.y * f.x - v2.x * f.y, h.x * af.y + h.y * af.x);
  return sx | sy | sz;
}
// The canonical triangle-against-box test (DESIGN.md §5 "Box overlaps"): Akenine-Möller's 13 axes in binary32 and in world space.
// A, ab, ac: the packet through the instance's o2w.  True: nothing separates the pair (a candidate).
__device__ __forceinline__ bool overlap_tri(F3 lo, F3 hi, F3 A, F3 ab, F3 ac) {
  const F3 B = add3(A, ab), C = add3(A, ac);
  const bool finite = finite_bits(A.x) && finite_bits(A.y) && finite_bits(A.z) && finite_bits(B.x) && finite_bits(B.y) && finite_bits(B.z) &&
                      finite_bits(C.x) && finite_bits(C.y) && finite_bits(C.z);
  // the box axes, on lo / hi themselves
  bool sep = (fminf(fminf(A.x, B.x), C.x) > hi.x) || (fmaxf(fmaxf(A.x, B.x), C.x) < lo.x) || (fminf(fminf(A.y, B.y), C.y) > hi.y) ||
             (fmaxf(fmaxf(A.y, B.y), C.y) < lo.y) || (fminf(fminf(A.z, B.z), C.z) > hi.z) || (fmaxf(fmaxf(A.z, B.z), C.z) < lo.z);
  if (sep || !finite) return false;   // (most packets of a leaf end here)
  const F3 c = mk3(0.5f * lo.x + 0.5f * hi.x, 0.5f * lo.y + 0.5f * hi.y, 0.5f * lo.z + 0.5f * hi.z);
  const F3 h = mk3(0.5f * hi.x - 0.5f * lo.x, 0.5f * hi.y - 0.5f * lo.y, 0.5f * hi.z - 0.5f * lo.z);
  const F3 v0 = sub3(A, c), v1 = sub3(B, c), v2 = sub3(C, c);
  const F3 f0 = sub3(v1, v0), f1 = sub3(v2, v1), f2 = sub3(v0, v2);
  const bool s0 = edge_separates(f0, v0, v1, v2, h), s1 = edge_separates(f1, v0, v1, v2, h), s2 = edge_separates(f2, v0, v1, v2, h);
  sep = s0 | s1 | s2;
  const F3 n = cross3(f0, f1);
  const float d = dot3(n, v0), r = dot3(h, mk3(__builtin_fabsf(n.x), __builtin_fabsf(n.y), __builtin_fabsf(n.z)));
  return !(sep | (__builtin_fabsf(d) > r));
}

// (inst, prim) before (bi, bp)
__device__ __forceinline__ bool id_before(int inst, int prim, int bi, int bp) { return inst < bi || (inst == bi && prim < bp); }

// the quantised box (wx, wy, wz) of a tree with dequantisation (q_lo, q_scale) against the query box [lo, hi]: closed, and a NaN opens
__device__ __forceinline__ bool box_touches(uint32_t wx, uint32_t wy, uint32_t wz, F3 lo, F3 hi, F3 q_lo, F3 q_scale) {
  F3 bl, bh;
  box_planes(wx, wy, wz, q_lo, q_scale, bl, bh);
  return !(bl.x > hi.x) && !(bh.x < lo.x) && !(bl.y > hi.y) && !(bh.y < lo.y) && !(bl.z > hi.z) && !(bh.z < lo.z);
}

// Entering instance I (k_overlap_boxes and k_collide_triangles alike): the dequantisation of its BLAS, and the inflated world box
// [qlo, qhi] replaced by the query of that tree (the head of this file).  s: the instance's entry of k_closest_scale's array.
__device__ __forceinline__ void overlap_enter_instance(const InstanceDev* I, float s, F3& qlo, F3& qhi, F3& q_lo, F3& q_scale) {
  const float INF = __builtin_inff();
  const float* w = I->w2o;
  q_lo = mk3(I->q_lo[0], I->q_lo[1], I->q_lo[2]); q_scale = mk3(I->q_scale[0], I->q_scale[1], I->q_scale[2]);
  // the object-space bound of the inflated world box's corners
  F3 mn = mk3(INF, INF, INF), mx = mk3(-INF, -INF, -INF);
  for (int k = 0; k < 8; k++) {
    const F3 p = xform_point(w, mk3((k & 1) ? qhi.x : qlo.x, (k & 2) ? qhi.y : qlo.y, (k & 4) ? qhi.z : qlo.z));
    mn = mk3(fminf(mn.x, p.x), fminf(mn.y, p.y), fminf(mn.z, p.z)); mx = mk3(fmaxf(mx.x, p.x), fmaxf(mx.y, p.y), fmaxf(mx.z, p.z));
  }
  // magnitudes: the mesh's planes, the terms of the corners' rows (they may cancel)
  const F3 cm = mk3(fmaxf(__builtin_fabsf(qlo.x), __builtin_fabsf(qhi.x)), fmaxf(__builtin_fabsf(qlo.y), __builtin_fabsf(qhi.y)),
                    fmaxf(__builtin_fabsf(qlo.z), __builtin_fabsf(qhi.z)));
  float om = 0.f;
  for (int k = 0; k < 3; k++) {
    om = fmaxf(om, fmaxf(__builtin_fabsf(I->q_lo[k]), __builtin_fabsf(__builtin_fmaf(65535.0f, I->q_scale[k], I->q_lo[k]))));
    om = fmaxf(om, __builtin_fabsf(w[4 * k]) * cm.x + __builtin_fabsf(w[4 * k + 1]) * cm.y + __builtin_fabsf(w[4 * k + 2]) * cm.z + __builtin_fabsf(w[4 * k + 3]));
  }
  // (fmaxf drops a NaN term: the sum of the corner bounds brings it back)
  const float chk = om + ((mn.x + mn.y + mn.z) + (mx.x + mx.y + mx.z)) * 0.0f;
  if (s > 0.0f && chk <= 3.0e38f) {
    const float so = OB_ABS * om;
    qlo = mk3(mn.x - so, mn.y - so, mn.z - so); qhi = mk3(mx.x + so, mx.y + so, mx.z + so);
  } else {   // a singular or non-finite transform, an unbounded slack: the instance's boxes do not prune
    qlo = mk3(-INF, -INF, -INF); qhi = mk3(INF, INF, INF);
  }
}

template <bool COUNT, bool LIST = false>
__device__ __forceinline__ void overlap_body(const OverlapArgs& a) {
  __shared__ int s_stack[4][STACK2_LDS][64];
  WalkStack st(s_stack, a.ovf_stack, a.sc.ovf_stride);
  WalkFeed feed;
  const uint32_t K = a.k;
  const bool prune = !LIST && a.counts == nullptr;
  uint32_t len = 0;                           // LIST: the row's length, from the offsets (0: a row that is not written)

  bool need = true;
  uint32_t bx = 0, count = 0;
  F3 wlo = mk3(0, 0, 0), whi = wlo;           // the box as given (the predicate's)
  F3 qlo = wlo, qhi = wlo;                    // the inflated query box in the space of the tree being walked
  float w_slack = 0.f;
  F3 q_lo = wlo, q_scale = wlo;               // dequantisation of that tree
  int last_inst = 0, last_prim = 0;           // the row's last entry once it is full
  int cur = REF_DONE, cur_inst = -1;
  IdRec* row = nullptr;
  unsigned long long cnt_nodes = 0, cnt_tris = 0;

  auto world_space = [&]() {
    qlo = mk3(wlo.x - w_slack, wlo.y - w_slack, wlo.z - w_slack); qhi = mk3(whi.x + w_slack, whi.y + w_slack, whi.z + w_slack);
    tlas_dequant(a.sc, q_lo, q_scale);
  };

  for (;;) {
    // ---- refill: idle lanes take the next boxes of the wave's chunk
    const uint32_t rec = feed.take(__ballot(need), a.cursor, a.n);
    if (need && rec != WALK_NONE) {
      bx = rec;
      const float4 r0 = ld_stream(&a.boxes[2u * (size_t)bx]), r1 = ld_stream(&a.boxes[2u * (size_t)bx + 1u]);
      wlo = mk3(r0.x, r0.y, r0.z); whi = mk3(r1.x, r1.y, r1.z);
      const bool valid = finite_bits(r0.x) && finite_bits(r0.y) && finite_bits(r0.z) && finite_bits(r1.x) && finite_bits(r1.y) && finite_bits(r1.z) &&
                         r0.x <= r1.x && r0.y <= r1.y && r0.z <= r1.z;
      const float mag = fmaxf(fmaxf(fmaxf(__builtin_fabsf(r0.x), __builtin_fabsf(r0.y)), __builtin_fabsf(r0.z)),
                              fmaxf(fmaxf(__builtin_fabsf(r1.x), __builtin_fabsf(r1.y)), __builtin_fabsf(r1.z)));
      w_slack = OB_ABS * fmaxf(tlas_magnitude(a.sc, mag), a.inst_scale[0]);
      world_space();
      cur_inst = -1; count = 0;
      st.reset(); cur = valid ? a.sc.tlas_root : REF_DONE;
      if (LIST) {   // the row the count walk measured: nothing to do for an empty one or one that ends beyond the capacity
        const unsigned long long o0 = a.offsets[bx], o1 = a.offsets[bx + 1u];
        len = o1 > a.capacity ? 0u : (uint32_t)(o1 - o0);
        if (len == 0u) cur = REF_DONE;
        row = a.ids + o0;
      } else row = a.ids + (size_t)bx * K;
      need = false;
    }
    if (__ballot(!need) == 0) break;   // every lane idle and the boxes used up

    // ---- interior nodes: every lane at one takes a visit; the trip repeats while most live lanes are interior
    for (;;) {
      if (cur >= 0) {
        uint4 Q0, Q1;
        walk_node(a.sc, cur, Q0, Q1);
        if (COUNT) cnt_nodes++;
        const bool h0 = box_present(Q0.x) && box_touches(Q0.x, Q0.y, Q0.z, qlo, qhi, q_lo, q_scale);
        const bool h1 = box_present(Q0.w) && box_touches(Q0.w, Q1.x, Q1.y, qlo, qhi, q_lo, q_scale);
        if (h0 && h1) { st.push((int)Q1.w); cur = (int)Q1.z; }
        else if (h0) cur = (int)Q1.z;
        else if (h1) cur = (int)Q1.w;
        else cur = st.pop();
      }
      if (walk_trip_done(need, cur)) break;
    }

    if (!need && cur < 0 && cur > REF_MARK && cur_inst >= 0) {
      // ---- BLAS leaf: the canonical test of every packet, in world space; a candidate is counted and, if it belongs in the row,
      // inserted in (inst, prim) order
      uint32_t first, nt;
      walk_leaf(cur, first, nt);
      const float* m = a.sc.inst[cur_inst].o2w;
      bool done = false;
      for (uint32_t j = 0; j < nt; j++) {
        const float4* tp = a.sc.tris + (size_t)(first + j) * 3;
        const float4 T0 = tp[0], T1 = tp[1], T2 = tp[2];
        const int prim = (int)__float_as_uint(T2.y);
        const bool full = K != 0u && count >= K;
        if (prune && full && !id_before(cur_inst, prim, last_inst, last_prim)) continue;   // (it could neither enter the row nor be counted)
        if (COUNT) cnt_tris++;
        if (!overlap_tri(wlo, whi, xform_point(m, mk3(T0.x, T0.y, T0.z)), xform_vec(m, mk3(T0.w, T1.x, T1.y)), xform_vec(m, mk3(T1.z, T1.w, T2.x)))) continue;
        if (LIST) {   // every candidate has its place (never beyond the row, whatever the walk finds): a short row by insertion, a long one in walk order
          if (count < len) {
            uint32_t p = count;
            if (len <= (uint32_t)RT_LIST_INSERT_MAX)
              while (p > 0u) {
                const IdRec o = row[p - 1u];
                if (!id_before(cur_inst, prim, o.inst, o.prim)) break;
                row[p] = o;
                p--;
              }
            IdRec id; id.inst = cur_inst; id.prim = prim;
            row[p] = id;
          }
          count++;
          continue;
        }
        const uint32_t e = count < K ? count : K;   // entries in the row
        count++;
        if (a.any) { done = true; break; }
        if (K == 0u) continue;                      // count-only
        uint32_t p = e;                             // the new entry's slot, found from the back
        if (e == K) {                               // full: it must precede the last entry, which falls off
          if (!id_before(cur_inst, prim, last_inst, last_prim)) continue;
          p = K - 1u;
        }
        while (p > 0u) {
          const IdRec o = row[p - 1u];
          if (!id_before(cur_inst, prim, o.inst, o.prim)) break;
          row[p] = o;
          p--;
        }
        IdRec id; id.inst = cur_inst; id.prim = prim;
        row[p] = id;
        if (count >= K) { const IdRec l = row[K - 1u]; last_inst = l.inst; last_prim = l.prim; }
      }
      if (done) cur = REF_DONE;
      else cur = st.pop();
    }
    if (!need && cur == REF_MARK) {
      // ---- leave the instance
      cur_inst = -1;
      world_space();
      cur = st.pop();
    }
    if (!need && cur < 0 && cur > REF_MARK && cur_inst < 0) {
      // ---- TLAS leaf: enter the instance if the call's mask lets it and, when pruning, the row could still take one of its triangles
      const int ii = ~cur;
      const InstanceDev* I = a.sc.inst + ii;
      if (((I->mask >> INST_WORLD_MASK_SHIFT) & a.cull_mask & 0xFFu) != 0u && !(prune && K != 0u && count >= K && ii > last_inst)) {
        overlap_enter_instance(I, a.inst_scale[1 + ii], qlo, qhi, q_lo, q_scale);
        st.push(REF_MARK);
        cur_inst = ii; cur = I->blas_root;
      } else cur = st.pop();
    }
    if (!need && cur == REF_DONE) {
      // ---- finished: the rest of the row empty, the count
      if (LIST) {   // (a long row goes to k_list_sort)
        if (len > (uint32_t)RT_LIST_INSERT_MAX) a.worklist[atomicAdd(a.work_count, 1u)] = bx;
      } else {
        IdRec none; none.inst = -1; none.prim = -1;
        for (uint32_t j = count < K ? count : K; j < K; j++) row[j] = none;
        if (a.counts) a.counts[bx] = count;
      }
      need = true;
    }
  }
  if (COUNT) walk_flush_counters(a.counters, cnt_nodes, cnt_tris);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_overlap_boxes(OverlapArgs a) { overlap_body<false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_overlap_boxes_count(OverlapArgs a) { overlap_body<true>(a); }

void launch_overlap_boxes(const SceneDev& sc, const float4* boxes, uint32_t cull_mask, const float* inst_scale, bool any, uint32_t k, void* ids, uint32_t* counts,
                          uint32_t n, int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s) {
  OverlapArgs a{};
  a.sc = sc; a.boxes = boxes; a.inst_scale = inst_scale; a.cull_mask = cull_mask; a.n = n; a.k = k; a.any = any ? 1u : 0u; a.ids = (IdRec*)ids; a.counts = counts;
  a.counters = counters; a.ovf_stack = ovf_stack;
  launch_walk(k_overlap_boxes, k_overlap_boxes_count, a, counters, counting, cfg, s);
}
