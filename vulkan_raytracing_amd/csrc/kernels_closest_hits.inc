// kernels_closest_hits.inc — included by kernels.hip after kernels_closest.inc (product and alt translation units alike).
// rt_closest_point_device_hits: for every query point the K nearest triangles within the record's radius and the number of triangles
// within it (a contact manifold, PhysX's overlapSphere count, the few nearest triangles to vote over).  k_closest_point's walk with
// k_query_hits' row in the place of the one best record: a walk of its own, no existing kernel changes.
//
//  * the arithmetic is k_closest_point's as it stands: closest_tri and box_bound (kernels_closest.inc) with CP_ABS / CP_REL and
//    closest_enter_instance (walk_nearest.inc), the scales of k_closest_scale; the deflated bound stays below the binary32 d2 of every triangle under the box, so which triangles
//    arrive at the leaf test does not depend on the tree (DESIGN.md §5 "K nearest triangles");
//  * candidates: d2 not NaN and d2 <= r_max * r_max — the set k_closest_point takes its minimum from;
//  * the row: in the lane's own row of the caller's hit array, kept sorted by (d2, inst, prim) by insertion from the back, d2 itself in
//    the t field until the finish step takes its root (two d2 may share a sqrtf: the order is d2's); only the count, the limit and the
//    row pointer live in registers (a runtime-indexed private array would be placed in scratch memory);
//  * the limit of the box tests: r_max * r_max, or the K-th entry's d2 once the row is full and no counts are wanted; a child is
//    skipped only when its bound EXCEEDS the limit, so a candidate at the K-th d2 with a smaller (inst, prim) still arrives and
//    replaces the K-th entry;
//  * the nearer child first, the farther one pushed.
#ifndef RT_CLOSEST_HITS_WAVES_PER_EU
#define RT_CLOSEST_HITS_WAVES_PER_EU 4   /* the record-level walks' budget */
#endif

struct ClosestHitsArgs {
  SceneDev sc;
  const float4* points;        // n records of 16 bytes: (p.xyz, r_max)
  const float* inst_scale;     // k_closest_scale's
  uint32_t cull_mask;
  uint32_t n;
  uint32_t k;                  // max_hits: 0..16 entries per row
  HitRec* hits;                // n * k records (k == 0: null)
  uint32_t* counts;            // n counts, or null (then the walk prunes)
  uint32_t* cursor;            // chunk cursor (zero before the launch)
  uint32_t* counters;          // the query's counter block (counting form: CNT_NODE_VISITS, CNT_TRI_TESTS)
  int32_t* ovf_stack;          // ovf_stride ints per thread of the grid
};

template <bool COUNT>
__device__ __forceinline__ void closest_hits_body(const ClosestHitsArgs& a) {
  __shared__ int s_stack[4][STACK2_LDS][64];
  WalkStack st(s_stack, a.ovf_stack, a.sc.ovf_stride);
  WalkFeed feed;
  const uint32_t K = a.k;
  const bool prune = a.counts == nullptr;

  bool need = true;
  uint32_t pt = 0, count = 0;
  F3 wp = mk3(0, 0, 0), q = wp;               // the point in world space; in the space of the tree being walked
  float w_slack = 0.f, slack = 0.f, scale2 = CP_REL;
  F3 q_lo = wp, q_scale = wp;                 // dequantisation of that tree
  float lim = 0.f;                            // the largest d2 still wanted: r_max * r_max, or the K-th entry's d2 (full row, pruning)
  int cur = REF_DONE, cur_inst = -1;
  HitRec* row = nullptr;
  unsigned long long cnt_nodes = 0, cnt_tris = 0;

  auto world_space = [&]() { q = wp; slack = w_slack; scale2 = CP_REL; tlas_dequant(a.sc, q_lo, q_scale); };

  for (;;) {
    // ---- refill: idle lanes take the next points of the wave's chunk
    const uint32_t rec = feed.take(__ballot(need), a.cursor, a.n);
    if (need && rec != WALK_NONE) {
      pt = rec;
      const float4 r = ld_stream(&a.points[pt]);
      wp = mk3(r.x, r.y, r.z);
      const bool valid = finite_bits(r.x) && finite_bits(r.y) && finite_bits(r.z) && r.w >= 0.0f;
      lim = r.w * r.w; count = 0;
      const float pmag = fmaxf(fmaxf(__builtin_fabsf(r.x), __builtin_fabsf(r.y)), __builtin_fabsf(r.z));
      w_slack = CP_ABS * fmaxf(fmaxf(pmag, tlas_magnitude(a.sc, 0.f)), a.inst_scale[0]);
      world_space();
      cur_inst = -1;
      st.reset(); cur = valid ? a.sc.tlas_root : REF_DONE;
      row = a.hits + (size_t)pt * K;
      need = false;
    }
    if (__ballot(!need) == 0) break;   // every lane idle and the points used up

    // ---- interior nodes: every lane at one takes a visit; the trip repeats while most live lanes are interior
    for (;;) {
      if (cur >= 0) {
        uint4 Q0, Q1;
        walk_node(a.sc, cur, Q0, Q1);
        if (COUNT) cnt_nodes++;
        const float b0 = box_bound(Q0.x, Q0.y, Q0.z, q, q_lo, q_scale, slack, scale2);
        const float b1 = box_bound(Q0.w, Q1.x, Q1.y, q, q_lo, q_scale, slack, scale2);
        // (!(b > lim): inclusive, and an unbounded limit opens all)
        const bool h0 = box_present(Q0.x) && !(b0 > lim);
        const bool h1 = box_present(Q0.w) && !(b1 > lim);
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
      // ---- BLAS leaf: the canonical test of every packet, in world space; a candidate is counted and, if it belongs in the row,
      // inserted in (d2, inst, prim) order (the t field holds d2 until the finish)
      uint32_t first, nt;
      walk_leaf(cur, first, nt);
      const float* m = a.sc.inst[cur_inst].o2w;
      for (uint32_t j = 0; j < nt; j++) {
        const float4* tp = a.sc.tris + (size_t)(first + j) * 3;
        const float4 T0 = tp[0], T1 = tp[1], T2 = tp[2];
        if (COUNT) cnt_tris++;
        float uu, vv;
        const float d2 = closest_tri(wp, xform_point(m, mk3(T0.x, T0.y, T0.z)), xform_vec(m, mk3(T0.w, T1.x, T1.y)), xform_vec(m, mk3(T1.z, T1.w, T2.x)), uu, vv);
        // (NaN is no candidate.  While it prunes, lim is at most r_max * r_max and what lies beyond it cannot enter the full row; the
        // count is then not reported)
        if (!(d2 <= lim)) continue;
        const int prim = (int)__float_as_uint(T2.y);
        const uint32_t e = count < K ? count : K;   // entries in the row
        count++;
        if (K == 0u) continue;                      // count-only
        uint32_t p = e;                             // the new entry's slot, found from the back
        if (e == K) {                               // full: it must precede the K-th entry, which falls off
          if (!hit_before(d2, cur_inst, prim, row[K - 1u])) continue;
          p = K - 1u;
        }
        while (p > 0u) {
          const HitRec o = row[p - 1u];
          if (!hit_before(d2, cur_inst, prim, o)) break;
          row[p] = o;
          p--;
        }
        HitRec h; h.t = d2; h.u = uu; h.v = vv; h.prim = prim; h.inst = cur_inst;
        row[p] = h;
        if (prune && count >= K) lim = row[K - 1u].t;
      }
      cur = st.pop();
    }
    if (!need && cur == REF_MARK) {
      // ---- leave the instance
      cur_inst = -1;
      world_space();
      cur = st.pop();
    }
    if (!need && cur < 0 && cur > REF_MARK && cur_inst < 0) {
      // ---- TLAS leaf: enter the instance if the call's mask lets it
      const int ii = ~cur;
      const InstanceDev* I = a.sc.inst + ii;
      if (((I->mask >> INST_WORLD_MASK_SHIFT) & a.cull_mask & 0xFFu) != 0u) {
        closest_enter_instance(I, a.inst_scale[1 + ii], wp, w_slack, q, q_lo, q_scale, slack, scale2);
        st.push(REF_MARK);
        cur_inst = ii; cur = I->blas_root;
      } else cur = st.pop();
    }
    if (!need && cur == REF_DONE) {
      // ---- finished: the distances of the filled entries, the rest of the row in the miss form with the radius as given, the count
      const uint32_t e = count < K ? count : K;
      for (uint32_t j = 0; j < e; j++) row[j].t = __builtin_sqrtf(row[j].t);
      HitRec miss; miss.t = ld_stream(&a.points[pt]).w; miss.u = 0.f; miss.v = 0.f; miss.prim = -1; miss.inst = -1;
      for (uint32_t j = e; j < K; j++) row[j] = miss;
      if (a.counts) a.counts[pt] = count;
      need = true;
    }
  }
  if (COUNT) walk_flush_counters(a.counters, cnt_nodes, cnt_tris);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_CLOSEST_HITS_WAVES_PER_EU))) void k_closest_hits(ClosestHitsArgs a) { closest_hits_body<false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_CLOSEST_HITS_WAVES_PER_EU))) void k_closest_hits_count(ClosestHitsArgs a) { closest_hits_body<true>(a); }

// k_closest_side over the n x k rows: record i belongs to point i / k
__global__ __launch_bounds__(256) void k_closest_hits_side(SceneDev sc, const float4* __restrict__ points, const HitRec* __restrict__ hits, uint32_t* __restrict__ attr,
                                                          uint32_t total, uint32_t k) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  attr[8u * (size_t)i + 7u] = closest_side_word(sc, points + i / k, hits[i]);
}

void launch_closest_hits(const SceneDev& sc, const float4* points, uint32_t cull_mask, const float* inst_scale, uint32_t n, uint32_t k, HitRec* hits, float4* attr,
                         uint32_t* counts, int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s) {
  ClosestHitsArgs a{};
  a.sc = sc; a.points = points; a.inst_scale = inst_scale; a.cull_mask = cull_mask; a.n = n; a.k = k; a.hits = hits; a.counts = counts; a.counters = counters;
  a.ovf_stack = ovf_stack;
  launch_walk(k_closest_hits, k_closest_hits_count, a, counters, counting, cfg, s);
  if (attr) {   // (k >= 1) the surface of every record of the flat rows, then the side words
    const uint32_t total = n * k;
    launch_hit_attr(sc, hits, attr, total, s);
    hipLaunchKernelGGL(k_closest_hits_side, dim3((total + 255u) / 256u), dim3(256), 0, s, sc, points, (const HitRec*)hits, reinterpret_cast<uint32_t*>(attr), total, k);
  }
}
