// walk_overlap.inc — included by kernels.hip before kernels_overlap.inc (product and alt translation units alike).
// The overlap family of record-level walks (walk_common.inc: the stack, the chunk feed, the trip exit, the counters), one lane per record:
// for every query record the triangles of the scene its predicate does not separate from it — their number and the smallest of them by
// (inst, prim), or (LIST) all of them.  One body, overlap_body<Shape, COUNT, REFS, LIST>, for k_overlap_boxes, k_collide_triangles,
// k_refs_collide and k_list_boxes / k_list_triangles / k_list_refs; a shape (kernels_overlap.inc: OverlapBox, kernels_triangles.inc:
// OverlapTriangle) carries what differs, the record and the leaf predicate:
//
//    static bool load(a, rec, wlo, whi, mag, against)     the record's bounds [wlo, whi], the largest magnitude of a coordinate and word
//                                                         11 (REFS: the instance to start at, or negative); true: a valid record
//    struct Leaf { Leaf(a, rec);                          what the predicate needs beside the bounds, read once per leaf ...
//                  bool touches(wlo, whi, A, ab, ac); }   ... and the canonical predicate against one packet through the instance's o2w
//    static bool own(a, rec, ii)                          REFS: instance ii is the source of a record against the others
//
//  * the node test is box against box on the dequantised planes, the query's bounds inflated (DESIGN.md §5 "Box overlaps"): in world
//    space by 2^-13 of the magnitudes that enter a candidate's world vertices (the bounds, the TLAS bounds, the row terms of every o2w:
//    word 0 of k_closest_scale's array); inside an instance the query is the bound of that inflated box's eight corners under w2o,
//    inflated again by 2^-13 of the mesh's bounds and of the row terms of w2o over the corners.  An instance with s_i == 0 (singular or
//    non-finite transform) or a non-finite bound gets an unbounded query: it does not prune.  A NaN opens the node;
//  * child 0 first, child 1 pushed;
//  * the list: in the lane's own row of the caller's id array, kept sorted by (inst, prim) by insertion; only the count and the row's
//    last entry live in registers, as in k_query_hits;
//  * pruning (no counts wanted): once the row is full, instances above the last entry's are not entered and triangles that do not
//    precede it are not tested; RT_OVERLAP_ANY ends the record at its first candidate;
//  * REFS (kernels_refs.inc): the records are k_refs_expand's, words 7 and 11 the source instance and `against`; a valid record with
//    against >= 0 starts at that instance's TLAS leaf with nothing beneath it, so the TLAS is never walked, and with against == -1 the
//    TLAS-leaf branch passes over the source instance;
//  * LIST (kernels_list.inc): every candidate into the row the offsets give, a short row by insertion, a long one in walk order;
//  * PAIRS (kernels_pairs.inc): a lane's item is one source triangle of an instance-pair record, held in the lane (Shape::Item); count
//    only, the count added to the record's 64-bit sum and the source primitive offered as its first; with `any` the record's word is the
//    flag that ends every item of the record.
#ifndef RT_OVERLAP_WAVES_PER_EU
#define RT_OVERLAP_WAVES_PER_EU 4   /* the record-level walks' budget */
#endif

struct IdRec { int32_t inst, prim; };   // 8 bytes, 4-byte aligned like the caller's rows

struct OverlapArgs {
  SceneDev sc;
  const float4* records;       // n records, as the shape reads them (32 or 48 bytes)
  const float* inst_scale;     // k_closest_scale: [0] the largest row-term magnitude of any instance's o2w, [1 + i] s_i
  uint32_t cull_mask;
  uint32_t n;
  uint32_t k;                  // max_ids: 0..16 entries per row
  uint32_t any;                // RT_OVERLAP_ANY: the count is 0 or 1, the record ends at its first candidate
  IdRec* ids;                  // n * k records (inst, prim) (k == 0: null)
  uint32_t* counts;            // n counts, or null (then the walk prunes)
  uint32_t* cursor;            // chunk cursor (zero before the launch)
  uint32_t* counters;          // the query's counter block (counting form: CNT_NODE_VISITS, CNT_TRI_TESTS)
  int32_t* ovf_stack;          // ovf_stride ints per thread of the grid
  // the LIST instantiations only; behind everything else, so that the other kernels read their arguments where they did
  const unsigned long long* offsets;   // n + 1 row starts: row i is ids[offsets[i] .. offsets[i + 1])
  unsigned long long capacity; // records of ids: a row that ends beyond it is not written
  uint32_t* worklist;          // the rows left in walk order (longer than RT_LIST_INSERT_MAX), for k_list_sort
  uint32_t* work_count;        // their number (zero before the launch)
  // the PAIRS instantiations only (offsets: the n + 1 starts of the records' work items)
  const int4* irefs;           // n instance-pair records (rt_inst_ref)
  unsigned long long* sums;    // n sums of counts; any: n words 0 or 1, the flag of the record
  uint32_t* first_p;           // n words: the smallest source primitive with a candidate (0xFFFFFFFF: none), or null
  uint32_t n_vert_floats;      // the floats of sc.verts
};
struct NoItem {};

constexpr float OB_ABS = 1.220703125e-04f;          // 2^-13: absolute slack per unit of magnitude

// (inst, prim) before (bi, bp)
__device__ __forceinline__ bool id_before(int inst, int prim, int bi, int bp) { return inst < bi || (inst == bi && prim < bp); }

// the quantised box (wx, wy, wz) of a tree with dequantisation (q_lo, q_scale) against the query box [lo, hi]: closed, and a NaN opens
__device__ __forceinline__ bool box_touches(uint32_t wx, uint32_t wy, uint32_t wz, F3 lo, F3 hi, F3 q_lo, F3 q_scale) {
  F3 bl, bh;
  box_planes(wx, wy, wz, q_lo, q_scale, bl, bh);
  return !(bl.x > hi.x) && !(bh.x < lo.x) && !(bl.y > hi.y) && !(bh.y < lo.y) && !(bl.z > hi.z) && !(bh.z < lo.z);
}

// Entering instance I: the dequantisation of its BLAS, and the inflated world box [qlo, qhi] replaced by the query of that tree (the
// head of this file).  s: the instance's entry of k_closest_scale's array.
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

template <class Shape, bool COUNT, bool REFS = false, bool LIST = false, bool PAIRS = false>
__device__ __forceinline__ void overlap_body(const OverlapArgs& a) {
  __shared__ int s_stack[4][STACK2_LDS][64];
  WalkStack st(s_stack, a.ovf_stack, a.sc.ovf_stride);
  WalkFeed feed;
  const uint32_t K = PAIRS ? 0u : a.k;
  const bool prune = !LIST && !PAIRS && a.counts == nullptr;
  uint32_t len = 0;                           // LIST: the row's length, from the offsets (0: a row that is not written)

  bool need = true;
  uint32_t bx = 0, count = 0;
  F3 wlo = mk3(0, 0, 0), whi = wlo;           // the record's bounds as given (the predicate's)
  F3 qlo = wlo, qhi = wlo;                    // the inflated bounds in the space of the tree being walked
  float w_slack = 0.f;
  F3 q_lo = wlo, q_scale = wlo;               // dequantisation of that tree
  int last_inst = 0, last_prim = 0;           // the row's last entry once it is full
  int cur = REF_DONE, cur_inst = -1;
  IdRec* row = nullptr;
  unsigned long long cnt_nodes = 0, cnt_tris = 0;
  uint32_t n_items = a.n;                     // PAIRS: the work items of all records, from the device
  if constexpr (PAIRS) n_items = (uint32_t)a.offsets[a.n];
  typename Shape::Item item;                  // PAIRS: the source triangle and its record

  auto world_space = [&]() {
    qlo = mk3(wlo.x - w_slack, wlo.y - w_slack, wlo.z - w_slack); qhi = mk3(whi.x + w_slack, whi.y + w_slack, whi.z + w_slack);
    tlas_dequant(a.sc, q_lo, q_scale);
  };

  for (;;) {
    // ---- refill: idle lanes take the next records of the wave's chunk
    const uint32_t rec = feed.take(__ballot(need), a.cursor, n_items);
    if (need && rec != WALK_NONE) {
      bx = rec;
      float mag;
      int against;
      bool valid;
      if constexpr (PAIRS) valid = Shape::load(a, bx, item, wlo, whi, mag, against) && !Shape::ended(a, item);
      else valid = Shape::load(a, bx, wlo, whi, mag, against);
      w_slack = OB_ABS * fmaxf(tlas_magnitude(a.sc, mag), a.inst_scale[0]);
      world_space();
      cur_inst = -1; count = 0;
      st.reset(); cur = valid ? a.sc.tlas_root : REF_DONE;
      if (REFS && valid && against >= 0) cur = ~against;   // (k_refs_expand: below n_inst)
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
      // ---- BLAS leaf: the canonical test of every packet, in world space; a candidate is counted and, if it belongs in the row,
      // inserted in (inst, prim) order
      uint32_t first, nt;
      walk_leaf(cur, first, nt);
      const float* m = a.sc.inst[cur_inst].o2w;
      const typename Shape::Leaf leaf(a, bx, item);
      bool done = false;
      if constexpr (PAIRS) if (Shape::ended(a, item)) { done = true; nt = 0u; }   // (another item of the record found a contact)
      for (uint32_t j = 0; j < nt; j++) {
        const float4* tp = a.sc.tris + (size_t)(first + j) * 3;
        const float4 T0 = tp[0], T1 = tp[1], T2 = tp[2];
        const int prim = (int)__float_as_uint(T2.y);
        const bool full = K != 0u && count >= K;
        if (prune && full && !id_before(cur_inst, prim, last_inst, last_prim)) continue;   // (it could neither enter the row nor be counted)
        if (COUNT) cnt_tris++;
        if (!leaf.touches(wlo, whi, xform_point(m, mk3(T0.x, T0.y, T0.z)), xform_vec(m, mk3(T0.w, T1.x, T1.y)), xform_vec(m, mk3(T1.z, T1.w, T2.x)))) continue;
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
      bool own = false;   // REFS: the source instance of a record against the others (the record read again)
      if constexpr (PAIRS) own = Shape::own(a, item, ii);
      else if constexpr (REFS) own = Shape::own(a, bx, ii);
      if (((I->mask >> INST_WORLD_MASK_SHIFT) & a.cull_mask & 0xFFu) != 0u && !(prune && K != 0u && count >= K && ii > last_inst) && !own) {
        overlap_enter_instance(I, a.inst_scale[1 + ii], qlo, qhi, q_lo, q_scale);
        st.push(REF_MARK);
        cur_inst = ii; cur = I->blas_root;
      } else cur = st.pop();
    }
    if (!need && cur == REF_DONE) {
      // ---- finished: the rest of the row empty, the count
      if constexpr (PAIRS) {
        if (count != 0u) Shape::finish(a, item, count);
      } else if (LIST) {   // (a long row goes to k_list_sort)
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

// The capped kernels of the family, which the shapes' files define (kernels_overlap.inc, kernels_triangles.inc, kernels_refs.inc), and
// their launch.  (launch_overlap_list: kernels_list.inc.)
__global__ void k_overlap_boxes(OverlapArgs), k_overlap_boxes_count(OverlapArgs), k_collide_triangles(OverlapArgs), k_collide_triangles_count(OverlapArgs),
    k_refs_collide(OverlapArgs), k_refs_collide_count(OverlapArgs);

static OverlapArgs overlap_args(const SceneDev& sc, const float4* records, uint32_t cull_mask, const float* inst_scale, void* ids, uint32_t n, int32_t* ovf_stack,
                                uint32_t* counters) {
  OverlapArgs a{};
  a.sc = sc; a.records = records; a.inst_scale = inst_scale; a.cull_mask = cull_mask; a.n = n; a.ids = (IdRec*)ids; a.counters = counters; a.ovf_stack = ovf_stack;
  return a;
}

void launch_overlap(OverlapShape shape, const SceneDev& sc, const float4* records, uint32_t cull_mask, const float* inst_scale, bool any, uint32_t k, void* ids,
                    uint32_t* counts, uint32_t n, int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s) {
  static void (*const kernels[3][2])(OverlapArgs) = {
      {k_overlap_boxes, k_overlap_boxes_count}, {k_collide_triangles, k_collide_triangles_count}, {k_refs_collide, k_refs_collide_count}};
  OverlapArgs a = overlap_args(sc, records, cull_mask, inst_scale, ids, n, ovf_stack, counters);
  a.k = k; a.any = any ? 1u : 0u; a.counts = counts;
  launch_walk(kernels[(int)shape][0], kernels[(int)shape][1], a, counters, counting, cfg, s);
}
