// kernels_triangles.inc — included by kernels.hip after kernels_overlap.inc (product and alt translation units alike).
// rt_overlap_triangles_device: for every query triangle the triangles of the scene that cut or touch it — their number and the smallest
// of them by (inst, prim).  The sixth record-level walk (walk_common.inc), one lane per query triangle:
//
//  * the node test is k_overlap_boxes' test applied to the query's bounds [min(P0, P1, P2), max(P0, P1, P2)]: box_touches, the same 2^-13
//    world slack, and overlap_enter_instance for the object-space query of an instance (kernels_overlap.inc, shared, not copied).  The
//    walk therefore visits the nodes and packets k_overlap_boxes visits for the bounding boxes;
//  * the triangle test is the canonical sequence of DESIGN.md §5 "Triangle overlaps" in world space (collide_tri): the bounds of the
//    candidate against the bounds of the query, then seventeen separating axes on vertices centred on P0.  It depends on the query
//    record, the instance record and the packet only;
//  * the lane keeps the query's bounds across the walk and reads the 48-byte record again at every leaf (resident in cache): nine
//    floats fewer beside the walk state;
//  * the row, the pruning, RT_OVERLAP_ANY and the finish are k_overlap_boxes'.

struct CollideArgs {
  SceneDev sc;
  const float4* tris;          // n records of 48 bytes: (P0.xyz, w3), (P1.xyz, w7), (P2.xyz, w11)
  const float* inst_scale;     // k_closest_scale: [0] the largest row-term magnitude of any instance's o2w, [1 + i] s_i
  uint32_t cull_mask;
  uint32_t n;
  uint32_t k;                  // max_ids: 0..16 entries per row
  uint32_t any;                // RT_OVERLAP_ANY
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

// one axis L: the query projects to 0, L.p1, L.p2 and the candidate to L.a, L.b, L.c (everything centred on P0).  Strict: a tie is not a
// separation; a zero axis projects everything to 0 and separates nothing; fminf / fmaxf pass over a NaN among numbers.
__device__ __forceinline__ bool collide_axis(F3 L, F3 p1, F3 p2, F3 a, F3 b, F3 c) {
  const float q1 = dot3(L, p1), q2 = dot3(L, p2), ta = dot3(L, a), tb = dot3(L, b), tc = dot3(L, c);
  const float qmin = fminf(fminf(0.0f, q1), q2), qmax = fmaxf(fmaxf(0.0f, q1), q2);
  const float tmin = fminf(fminf(ta, tb), tc), tmax = fmaxf(fmaxf(ta, tb), tc);
  return (qmin > tmax) | (qmax < tmin);
}

// The canonical triangle-against-triangle test (DESIGN.md §5 "Triangle overlaps"), binary32, world space, every axis evaluated.
// [wlo, whi]: the query's bounds; A, ab, ac: the packet through the instance's o2w.  True: nothing separates the pair (a candidate).
__device__ __forceinline__ bool collide_tri(F3 wlo, F3 whi, F3 P0, F3 P1, F3 P2, F3 A, F3 ab, F3 ac) {
  const F3 B = add3(A, ab), C = add3(A, ac);
  const bool finite = finite_bits(A.x) && finite_bits(A.y) && finite_bits(A.z) && finite_bits(B.x) && finite_bits(B.y) && finite_bits(B.z) &&
                      finite_bits(C.x) && finite_bits(C.y) && finite_bits(C.z);
  // step 2: the bounds of the query, on the vertices themselves
  bool sep = (fminf(fminf(A.x, B.x), C.x) > whi.x) || (fmaxf(fmaxf(A.x, B.x), C.x) < wlo.x) || (fminf(fminf(A.y, B.y), C.y) > whi.y) ||
             (fmaxf(fmaxf(A.y, B.y), C.y) < wlo.y) || (fminf(fminf(A.z, B.z), C.z) > whi.z) || (fmaxf(fmaxf(A.z, B.z), C.z) < wlo.z);
  if (sep || !finite) return false;   // (most packets of a leaf end here)
  const F3 p1 = sub3(P1, P0), p2 = sub3(P2, P0);
  const F3 a = sub3(A, P0), b = sub3(B, P0), c = sub3(C, P0);
  const F3 g0 = p1, g1 = sub3(p2, p1), g2 = p2;
  const F3 f0 = sub3(b, a), f1 = sub3(c, b), f2 = sub3(a, c);
  const F3 n = cross3(g0, g2), m = cross3(f0, f1);
  sep = collide_axis(n, p1, p2, a, b, c);
  sep |= collide_axis(m, p1, p2, a, b, c);
  sep |= collide_axis(cross3(g0, f0), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g0, f1), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g0, f2), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g1, f0), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g1, f1), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g1, f2), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g2, f0), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g2, f1), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g2, f2), p1, p2, a, b, c);
  sep |= collide_axis(cross3(n, g0), p1, p2, a, b, c);
  sep |= collide_axis(cross3(n, g1), p1, p2, a, b, c);
  sep |= collide_axis(cross3(n, g2), p1, p2, a, b, c);
  sep |= collide_axis(cross3(m, f0), p1, p2, a, b, c);
  sep |= collide_axis(cross3(m, f1), p1, p2, a, b, c);
  sep |= collide_axis(cross3(m, f2), p1, p2, a, b, c);
  return !sep;
}

// REFS (kernels_refs.inc, rt_overlap_scene_triangles_device): the records are k_refs_expand's, words 7 and 11 the source instance and
// `against`; a valid record with against >= 0 starts at that instance's TLAS leaf with nothing beneath it, so the TLAS is never walked,
// and with against == -1 the TLAS-leaf branch passes over the source instance.  Everything else is shared.
template <bool COUNT, bool REFS = false, bool LIST = false>
__device__ __forceinline__ void collide_body(const CollideArgs& a) {
  __shared__ int s_stack[4][STACK2_LDS][64];
  WalkStack st(s_stack, a.ovf_stack, a.sc.ovf_stride);
  WalkFeed feed;
  const uint32_t K = a.k;
  const bool prune = !LIST && a.counts == nullptr;
  uint32_t len = 0;                           // LIST: the row's length, from the offsets (0: a row that is not written)

  bool need = true;
  uint32_t bx = 0, count = 0;
  F3 wlo = mk3(0, 0, 0), whi = wlo;           // the query's bounds (step 2 of the predicate; the node test's box)
  F3 qlo = wlo, qhi = wlo;                    // the inflated bounds in the space of the tree being walked
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
    // ---- refill: idle lanes take the next query triangles of the wave's chunk
    const uint32_t rec = feed.take(__ballot(need), a.cursor, a.n);
    if (need && rec != WALK_NONE) {
      bx = rec;
      const float4* qp = a.tris + 3u * (size_t)bx;
      const float4 r0 = ld_stream(&qp[0]), r1 = ld_stream(&qp[1]), r2 = ld_stream(&qp[2]);
      wlo = mk3(fminf(fminf(r0.x, r1.x), r2.x), fminf(fminf(r0.y, r1.y), r2.y), fminf(fminf(r0.z, r1.z), r2.z));
      whi = mk3(fmaxf(fmaxf(r0.x, r1.x), r2.x), fmaxf(fmaxf(r0.y, r1.y), r2.y), fmaxf(fmaxf(r0.z, r1.z), r2.z));
      const bool valid = finite_bits(r0.x) && finite_bits(r0.y) && finite_bits(r0.z) && finite_bits(r1.x) && finite_bits(r1.y) && finite_bits(r1.z) &&
                         finite_bits(r2.x) && finite_bits(r2.y) && finite_bits(r2.z);
      const float mag = fmaxf(fmaxf(fmaxf(__builtin_fabsf(wlo.x), __builtin_fabsf(wlo.y)), __builtin_fabsf(wlo.z)),
                              fmaxf(fmaxf(__builtin_fabsf(whi.x), __builtin_fabsf(whi.y)), __builtin_fabsf(whi.z)));
      w_slack = OB_ABS * fmaxf(tlas_magnitude(a.sc, mag), a.inst_scale[0]);
      world_space();
      cur_inst = -1; count = 0;
      st.reset(); cur = valid ? a.sc.tlas_root : REF_DONE;
      if (REFS && valid && (int)__float_as_uint(r2.w) >= 0) cur = ~(int)__float_as_uint(r2.w);   // (k_refs_expand: below n_inst)
      if (LIST) {   // the row the count walk measured: nothing to do for an empty one or one that ends beyond the capacity
        const unsigned long long o0 = a.offsets[bx], o1 = a.offsets[bx + 1u];
        len = o1 > a.capacity ? 0u : (uint32_t)(o1 - o0);
        if (len == 0u) cur = REF_DONE;
        row = a.ids + o0;
      } else row = a.ids + (size_t)bx * K;
      need = false;
    }
    if (__ballot(!need) == 0) break;   // every lane idle and the records used up

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
      // ---- BLAS leaf: the canonical test of every packet, in world space, against the record read again; a candidate is counted
      // and, if it belongs in the row, inserted in (inst, prim) order
      uint32_t first, nt;
      walk_leaf(cur, first, nt);
      const float* m = a.sc.inst[cur_inst].o2w;
      const float4* qp = a.tris + 3u * (size_t)bx;
      const float4 r0 = qp[0], r1 = qp[1], r2 = qp[2];
      const F3 P0 = mk3(r0.x, r0.y, r0.z), P1 = mk3(r1.x, r1.y, r1.z), P2 = mk3(r2.x, r2.y, r2.z);
      bool done = false;
      for (uint32_t j = 0; j < nt; j++) {
        const float4* tp = a.sc.tris + (size_t)(first + j) * 3;
        const float4 T0 = tp[0], T1 = tp[1], T2 = tp[2];
        const int prim = (int)__float_as_uint(T2.y);
        const bool full = K != 0u && count >= K;
        if (prune && full && !id_before(cur_inst, prim, last_inst, last_prim)) continue;   // (it could neither enter the row nor be counted)
        if (COUNT) cnt_tris++;
        if (!collide_tri(wlo, whi, P0, P1, P2, xform_point(m, mk3(T0.x, T0.y, T0.z)), xform_vec(m, mk3(T0.w, T1.x, T1.y)), xform_vec(m, mk3(T1.z, T1.w, T2.x)))) continue;
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
      bool own = false;   // REFS: the source instance of a record against the others (words 7 and 11, read again)
      if (REFS) {
        const float4* qp = a.tris + 3u * (size_t)bx;
        own = (int)__float_as_uint(qp[2].w) < 0 && ii == (int)__float_as_uint(qp[1].w);
      }
      if (((I->mask >> INST_WORLD_MASK_SHIFT) & a.cull_mask & 0xFFu) != 0u && !(prune && K != 0u && count >= K && ii > last_inst) && !own) {
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

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_collide_triangles(CollideArgs a) { collide_body<false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_collide_triangles_count(CollideArgs a) { collide_body<true>(a); }

void launch_collide_triangles(const SceneDev& sc, const float4* tris, uint32_t cull_mask, const float* inst_scale, bool any, uint32_t k, void* ids, uint32_t* counts,
                              uint32_t n, int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s) {
  CollideArgs a{};
  a.sc = sc; a.tris = tris; a.inst_scale = inst_scale; a.cull_mask = cull_mask; a.n = n; a.k = k; a.any = any ? 1u : 0u; a.ids = (IdRec*)ids; a.counts = counts;
  a.counters = counters; a.ovf_stack = ovf_stack;
  launch_walk(k_collide_triangles, k_collide_triangles_count, a, counters, counting, cfg, s);
}
