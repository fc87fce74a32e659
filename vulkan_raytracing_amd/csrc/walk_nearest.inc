// walk_nearest.inc — included by kernels.hip before kernels_closest.inc (product and alt translation units alike).
// The nearest-pair family of record-level walks (walk_common.inc: the stack, the chunk feed, the trip exit, the counters), one lane per
// record: for every query record the nearest pair of a point of the record and a point of the scene's surface within the record's
// radius.  One body, nearest_body<Shape, COUNT, REFS>, for k_closest_point, k_closest_segment, k_closest_triangle and k_refs_nearest; a
// shape (kernels_closest.inc: NearestPoint, kernels_segment.inc: NearestSegment, kernels_triangle.inc: NearestTriangle) carries what
// differs: the record in world space, its form in the space of the tree being walked, the node test, the leaf test and the result words
// beside the hit record:
//
//    static constexpr uint32_t STRIDE                   float4 per record (r_max is word 3)
//    struct Params                                      the result words of one candidate beside (d2, u, v); all zero on a miss
//    bool load(a, rec, r_max, pmag, against)            the record into world space; the largest magnitude of a coordinate and word 11
//                                                       (REFS: the instance to start at, or negative); true: a valid record
//    void to_world()                                    the walked-space form from the world-space record
//    F3 enter(I)                                        the same through I->w2o; returns the per-component largest magnitude of the
//                                                       record's points, which the slack of closest_enter_instance reads
//    void reach(best, scale2)                           after every change of best or of the walked space: the reach of the best d2 in
//                                                       the walked space's units, for a shape whose node test uses it
//    bool open(wx, wy, wz, q_lo, q_scale, slack, scale2, best, b)   the node test: b, the deflated squared lower bound that orders the
//                                                       children; true: the box may hold a pair no farther than best.  A NaN opens
//    float test(a, ab, ac, u, v, params)                the canonical leaf test against one packet through the instance's o2w: d2
//    static void store(a, rec, params)                  the result words into a.params
//    bool own(a, rec, ii)                               REFS: instance ii is the source of a record against the others
//
//  * distances inside an instance are multiplied by s_i <= sigma_min(linear part of o2w) (k_closest_scale), which makes them lower bounds
//    on world distances under any affine instance;
//  * bounds are deflated (DESIGN.md §5 "Closest points"): every axis distance by an absolute slack 2^-16 of the magnitudes that enter the
//    canonical d2 (the record's points, the planes, the rows of the transforms), the sum of squares by 1 - 2^-13, so that a bound stays
//    below the BINARY32 d2 of every triangle under the box; a subtree is skipped only when its bound EXCEEDS the best d2 (ties arrive);
//  * the nearer child first, the farther one pushed;
//  * the leaf test depends on the record, the instance record and the packet only, so the result is the minimum of the key
//    (d2, inst, prim) whatever the tree;
//  * REFS (kernels_refs.inc): the records are k_refs_expand's; a valid record with against >= 0 (word 11) starts at that instance's TLAS
//    leaf, one against the others passes over its source instance (word 7);
//  * PAIRS (kernels_pairs.inc): a lane's item is one source triangle of an instance-pair record, and the bound is shared: `best` is the
//    smaller of the lane's own best d2 and the smallest d2 any lane of the record has published (PairNearest::shared).  No hit is
//    kept: the key names the winning source triangle, and the by-reference call over it makes the answer.

struct NearestArgs {
  SceneDev sc;
  const float4* records;       // n records of Shape::STRIDE float4, r_max in word 3
  const float* inst_scale;     // k_closest_scale: [0] the largest row-term magnitude of any instance's o2w, [1 + i] s_i
  uint32_t cull_mask;
  uint32_t n;
  HitRec* hits;                // n records
  float* params;               // the shape's result words per record (zero on a miss), or null; the point walk has none
  uint32_t* cursor;            // chunk cursor (zero before the launch)
  uint32_t* counters;          // the query's counter block (counting form: CNT_NODE_VISITS, CNT_TRI_TESTS)
  int32_t* ovf_stack;          // ovf_stride ints per thread of the grid
  // the PAIRS instantiations only; behind everything else, so that the other kernels read their arguments where they did
  const int4* irefs;           // n instance-pair records (rt_inst_ref)
  const unsigned long long* offsets;   // n + 1 starts of the records' work items (offsets[n]: their number)
  unsigned long long* keys;    // n keys: the bits of the smallest published d2 << 32 | its smallest source primitive
  uint32_t n_vert_floats;      // the floats of sc.verts
};

constexpr float CP_ABS = 1.52587890625e-05f;       // 2^-16: absolute slack per unit of magnitude
constexpr float CP_REL = 0.9998779296875f;         // 1 - 2^-13: factor on the squared bound

// The entry of instance I (s: its scale of k_closest_scale) by the closest-family walks (this body, k_closest_hits): the world point wp
// into object space (q), the dequantisation of the mesh's tree, and the slack of both spaces in object units (w_slack: the walk's
// world-space slack) with the factor on the squared bound.  The slack formula reads |wp| only.
__device__ __forceinline__ void closest_enter_instance(const InstanceDev* I, float s, F3 wp, float w_slack, F3& q, F3& q_lo, F3& q_scale, float& slack, float& scale2) {
  const float* w = I->w2o; const float* o = I->o2w;
  q = xform_point(w, wp);
  q_lo = mk3(I->q_lo[0], I->q_lo[1], I->q_lo[2]); q_scale = mk3(I->q_scale[0], I->q_scale[1], I->q_scale[2]);
  // magnitudes: the mesh's planes, the terms of q's rows (they may cancel), the terms of o2w's rows over the mesh's bounds
  const F3 bm = mk3(fmaxf(__builtin_fabsf(q_lo.x), __builtin_fabsf(__builtin_fmaf(65535.0f, q_scale.x, q_lo.x))),
                    fmaxf(__builtin_fabsf(q_lo.y), __builtin_fabsf(__builtin_fmaf(65535.0f, q_scale.y, q_lo.y))),
                    fmaxf(__builtin_fabsf(q_lo.z), __builtin_fabsf(__builtin_fmaf(65535.0f, q_scale.z, q_lo.z))));
  const F3 ap = mk3(__builtin_fabsf(wp.x), __builtin_fabsf(wp.y), __builtin_fabsf(wp.z));
  float om = fmaxf(fmaxf(bm.x, bm.y), bm.z), wm = w_slack;
  for (int r = 0; r < 3; r++) {
    om = fmaxf(om, __builtin_fabsf(w[4 * r]) * ap.x + __builtin_fabsf(w[4 * r + 1]) * ap.y + __builtin_fabsf(w[4 * r + 2]) * ap.z + __builtin_fabsf(w[4 * r + 3]));
    wm = fmaxf(wm, CP_ABS * (__builtin_fabsf(o[4 * r]) * bm.x + __builtin_fabsf(o[4 * r + 1]) * bm.y + __builtin_fabsf(o[4 * r + 2]) * bm.z + __builtin_fabsf(o[4 * r + 3])));
  }
  slack = CP_ABS * om + wm / s;   // (s == 0: an infinite slack, every bound 0)
  scale2 = CP_REL * (s * s);
}

template <class Shape, bool COUNT, bool REFS = false, bool PAIRS = false>
__device__ __forceinline__ void nearest_body(const NearestArgs& a) {
  __shared__ int s_stack[4][STACK2_LDS][64];
  WalkStack st(s_stack, a.ovf_stack, a.sc.ovf_stride);
  WalkFeed feed;
  constexpr int NONE = 0x7FFFFFFF;            // best_inst / best_prim before the first candidate: every (inst, prim) precedes it

  bool need = true;
  uint32_t pt = 0;
  Shape sh;                                   // the record in world space and in the space of the tree being walked
  float w_slack = 0.f, slack = 0.f, scale2 = CP_REL;
  F3 q_lo = mk3(0, 0, 0), q_scale = q_lo;     // dequantisation of that tree
  float best = 0.f, best_u = 0.f, best_v = 0.f;
  typename Shape::Params best_p;
  int best_prim = NONE, best_inst = NONE;
  int cur = REF_DONE, cur_inst = -1;
  unsigned long long cnt_nodes = 0, cnt_tris = 0;
  uint32_t n_items = a.n;                     // PAIRS: the work items of all records, from the device
  if constexpr (PAIRS) n_items = (uint32_t)a.offsets[a.n];

  auto world_space = [&]() {
    sh.to_world();
    slack = w_slack; scale2 = CP_REL; tlas_dequant(a.sc, q_lo, q_scale);
    sh.reach(best, scale2);
  };

  for (;;) {
    // ---- refill: idle lanes take the next records of the wave's chunk
    const uint32_t rec = feed.take(__ballot(need), a.cursor, n_items);
    if (need && rec != WALK_NONE) {
      pt = rec;
      float r_max, pmag;
      int against;
      const bool valid = sh.load(a, pt, r_max, pmag, against);
      best = r_max * r_max;
      if constexpr (PAIRS) best = fminf(best, sh.shared(a));   // (never above r_max * r_max: the key starts there)
      best_u = 0.f; best_v = 0.f; best_p = typename Shape::Params(); best_prim = NONE; best_inst = NONE;
      w_slack = CP_ABS * fmaxf(fmaxf(pmag, tlas_magnitude(a.sc, 0.f)), a.inst_scale[0]);
      world_space();
      cur_inst = -1;
      st.reset(); cur = valid ? a.sc.tlas_root : REF_DONE;
      if (REFS && valid && against >= 0) cur = ~against;   // (k_refs_expand: below n_inst)
      need = false;
    }
    if (__ballot(!need) == 0) break;   // every lane idle and the records used up

    // ---- interior nodes: every lane at one takes a visit; the trip repeats while most live lanes are interior
    for (;;) {
      if (cur >= 0) {
        uint4 Q0, Q1;
        walk_node(a.sc, cur, Q0, Q1);
        if (COUNT) cnt_nodes++;
        float b0, b1;
        const bool h0 = sh.open(Q0.x, Q0.y, Q0.z, q_lo, q_scale, slack, scale2, best, b0) && box_present(Q0.x);
        const bool h1 = sh.open(Q0.w, Q1.x, Q1.y, q_lo, q_scale, slack, scale2, best, b1) && box_present(Q0.w);
        if (h0 && h1) {
          const bool swap = b1 < b0;
          st.push(swap ? (int)Q1.z : (int)Q1.w);
          cur = swap ? (int)Q1.w : (int)Q1.z;
        } else if (h0) cur = (int)Q1.z;
        else if (h1) cur = (int)Q1.w;
        else cur = st.pop();
      }
      if (walk_trip_done(need, cur)) break;
    }

    if (!need && cur < 0 && cur > REF_MARK && cur_inst >= 0) {
      // ---- BLAS leaf: the canonical test of every packet, in world space; the smallest key (d2, inst, prim) stays
      uint32_t first, nt;
      walk_leaf(cur, first, nt);
      const float* o = a.sc.inst[cur_inst].o2w;
      bool mine = false;   // PAIRS: best is a d2 of this leaf, to be published
      for (uint32_t j = 0; j < nt; j++) {
        const float4* tp = a.sc.tris + (size_t)(first + j) * 3;
        const float4 T0 = tp[0], T1 = tp[1], T2 = tp[2];
        if (COUNT) cnt_tris++;
        float uu, vv;
        typename Shape::Params pp;
        const float d2 = sh.test(xform_point(o, mk3(T0.x, T0.y, T0.z)), xform_vec(o, mk3(T0.w, T1.x, T1.y)), xform_vec(o, mk3(T1.z, T1.w, T2.x)), uu, vv, pp);
        const int prim = (int)__float_as_uint(T2.y);
        if constexpr (PAIRS) {   // no farther than the record's bound (a tie too: this source primitive may be the smaller one)
          if (d2 <= best) { best = d2; mine = true; }
          continue;
        }
        if (d2 < best || (d2 == best && (cur_inst < best_inst || (cur_inst == best_inst && prim < best_prim)))) {
          best = d2; best_u = uu; best_v = vv; best_p = pp; best_prim = prim; best_inst = cur_inst;
        }
      }
      if constexpr (PAIRS) {
        if (mine) sh.publish(a, best);
        best = fminf(best, sh.shared(a));
      }
      sh.reach(best, scale2);
      cur = st.pop();
    }
    if (!need && cur == REF_MARK) {
      // ---- leave the instance
      cur_inst = -1;
      world_space();
      cur = st.pop();
    }
    if (!need && cur < 0 && cur > REF_MARK && cur_inst < 0) {
      // ---- TLAS leaf: enter the instance if the call's mask lets it (the record -> object space, the slack of both spaces in object units)
      const int ii = ~cur;
      const InstanceDev* I = a.sc.inst + ii;
      bool own = false;   // REFS: the source instance of a record against the others (the record read again)
      if constexpr (REFS) own = sh.own(a, pt, ii);
      if (((I->mask >> INST_WORLD_MASK_SHIFT) & a.cull_mask & 0xFFu) != 0u && !own) {
        // (the object-space point closest_enter_instance returns for the magnitudes is not used: the shape holds itself)
        F3 unused;
        closest_enter_instance(I, a.inst_scale[1 + ii], sh.enter(I), w_slack, unused, q_lo, q_scale, slack, scale2);
        if constexpr (PAIRS) best = fminf(best, sh.shared(a));
        sh.reach(best, scale2);
        st.push(REF_MARK);
        cur_inst = ii; cur = I->blas_root;
      } else cur = st.pop();
    }
    if (!need && cur == REF_DONE) {
      // ---- finished: the record, or the miss form with the radius as given (read again)
      if constexpr (PAIRS) { need = true; continue; }   // (what the item found is in the record's key)
      HitRec h;
      if (best_inst != NONE) { h.t = __builtin_sqrtf(best); h.u = best_u; h.v = best_v; h.prim = best_prim; h.inst = best_inst; }
      else { h.t = ld_stream(&a.records[Shape::STRIDE * (size_t)pt]).w; h.u = 0.f; h.v = 0.f; h.prim = -1; h.inst = -1; best_p = typename Shape::Params(); }
      a.hits[pt] = h;
      Shape::store(a, pt, best_p);
      need = true;
    }
  }
  if (COUNT) walk_flush_counters(a.counters, cnt_nodes, cnt_tris);
}

// The kernels of the family, which the shapes' files define (kernels_closest.inc, kernels_segment.inc, kernels_triangle.inc,
// kernels_refs.inc), and their launch
__global__ void k_closest_point(NearestArgs), k_closest_point_count(NearestArgs), k_closest_segment(NearestArgs), k_closest_segment_count(NearestArgs),
    k_closest_triangle(NearestArgs), k_closest_triangle_count(NearestArgs), k_refs_nearest(NearestArgs), k_refs_nearest_count(NearestArgs);

void launch_nearest(NearestShape shape, const SceneDev& sc, const float4* records, uint32_t cull_mask, const float* inst_scale, HitRec* hits, float* params, uint32_t n,
                    int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s) {
  static void (*const kernels[4][2])(NearestArgs) = {{k_closest_point, k_closest_point_count}, {k_closest_segment, k_closest_segment_count},
                                                     {k_closest_triangle, k_closest_triangle_count}, {k_refs_nearest, k_refs_nearest_count}};
  NearestArgs a{};
  a.sc = sc; a.records = records; a.inst_scale = inst_scale; a.cull_mask = cull_mask; a.n = n; a.hits = hits; a.params = params;
  a.counters = counters; a.ovf_stack = ovf_stack;
  launch_walk(kernels[(int)shape][0], kernels[(int)shape][1], a, counters, counting, cfg, s);
}
