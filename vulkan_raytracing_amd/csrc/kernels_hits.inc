// kernels_hits.inc — included by kernels.hip (product and alt translation units alike).
// rt_intersect_device_hits: the K nearest accepted candidates of every ray and the number of them (VK_KHR_ray_query's
// rayQueryProceedEXT loop in data form).  A record-level walk of its own (walk_common.inc: the stack, the chunk feed, the trip exit),
// not a mode of trace_body: the frame kernels and the k_trace query instantiations stay exactly what they were.
//
//  * one lane per ray, without the phased loop of k_trace;
//  * the quantised BVH2 with the far-ray logic always on (origins are arbitrary): slab_q / slab_q_far, a far ray in world space opens
//    every TLAS child, exactly as trace_body's generic visit (interior_step);
//  * the instance rules of MODE_QUERY_FLAGS (query_enters) and its facing cull (tri_test_facing) over the ray's own [tmin, tmax];
//    TERMINATE_ON_FIRST_HIT is ignored, every accepted candidate counts;
//  * the list: in the lane's own row of the caller's hit array, kept sorted by (t, inst, prim) by insertion; only the count and
//    the K-th entry's t live in registers (a runtime-indexed private array would be placed in scratch memory);
//  * pruning (no counts wanted): once the row is full, boxes are tested up to the K-th entry's t, inclusive, so a candidate at that t
//    with a smaller (inst, prim) still reaches the insertion, which replaces the K-th entry.
#ifndef RT_HITS_WAVES_PER_EU
#define RT_HITS_WAVES_PER_EU 4   /* the record-level walks' budget */
#endif

struct HitsArgs {
  SceneDev sc;
  const float4* rays;          // n rays, 32 bytes each: (o.xyz, tmin), (d.xyz, tmax)
  const uint32_t* ray_words;   // n per-ray words (flags | cull mask << 24), or null: every word 0xFF000000
  uint32_t query_word;         // the call's ray flags | cull mask << 24
  uint32_t n;
  uint32_t k;                  // max_hits: 0..16 entries per row
  HitRec* hits;                // n * k records (k == 0: null)
  uint32_t* counts;            // n counts, or null (then the walk prunes)
  uint32_t* cursor;            // chunk cursor (zero before the launch)
  int32_t* ovf_stack;          // ovf_stride ints per thread of the grid
};

// (t, inst, prim) of a before that of b: the closest-hit tie rule (DESIGN.md §3)
__device__ __forceinline__ bool hit_before(float t, int inst, int prim, const HitRec& b) {
  return t < b.t || (t == b.t && (inst < b.inst || (inst == b.inst && prim < b.prim)));
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_HITS_WAVES_PER_EU))) void k_query_hits(HitsArgs a) {
  __shared__ int s_stack[4][STACK2_LDS][64];
  WalkStack st(s_stack, a.ovf_stack, a.sc.ovf_stride);
  WalkFeed feed;
  const uint32_t K = a.k;
  const bool prune = a.counts == nullptr;

  // per-lane ray state
  bool need = true;
  uint32_t ray = 0, count = 0, qword = 0;
  float tmin = 0.f, tmax = 0.f, lim = 0.f;   // lim: the box tests' upper limit (tmax, or the K-th entry's t once the row is full)
  F3 wo = mk3(0, 0, 0), wd = mk3(0, 0, 1), co = wo, cd = wd, qs = mk3(1, 1, 1), qb = mk3(0, 0, 0);
  uint3 rot = make_uint3(0u, 0u, 0u);
  bool far = false;
  int cur = REF_DONE, cur_inst = -1;
  HitRec* row = nullptr;

  auto world_space = [&]() {
    quant_space(wo, wd, a.sc.tlas_q_lo, a.sc.tlas_q_scale, qs, qb, rot); far = quant_far_o(wo, a.sc.tlas_q_lo, a.sc.tlas_q_scale);
  };

  for (;;) {
    // ---- refill: idle lanes take the next rays of the wave's chunk
    const uint32_t rec = feed.take(__ballot(need), a.cursor, a.n);
    if (need && rec != WALK_NONE) {
      ray = rec;
      const float4 ro = ld_stream(&a.rays[2u * (size_t)ray]), rd = ld_stream(&a.rays[2u * (size_t)ray + 1u]);
      const uint32_t w = a.ray_words ? (uint32_t)ld_stream(reinterpret_cast<const int*>(a.ray_words) + ray) : 0xFF000000u;
      qword = ((a.query_word | w) & QF_FLAGS) | (a.query_word & w & 0xFF000000u);
      tmin = ro.w; tmax = rd.w; lim = tmax;
      wo = mk3(ro.x, ro.y, ro.z); wd = mk3(rd.x, rd.y, rd.z);
      co = wo; cd = wd;
      world_space();
      cur_inst = -1; count = 0;
      st.reset(); cur = a.sc.tlas_root;
      row = a.hits + (size_t)ray * K;
      need = false;
    }
    if (__ballot(!need) == 0) break;   // every lane idle and the rays used up

    // ---- interior nodes: every lane at one takes a visit; the trip repeats while most live lanes are interior
    for (;;) {
      if (cur >= 0) {
        uint4 Q0, Q1;
        walk_node(a.sc, cur, Q0, Q1);
        float t0, t1;
        const bool open_all = far && cur_inst < 0;   // (a far ray in world space: the TLAS does not cull, trace_body's interior_step)
        const bool h0 = open_all ? box_present(Q0.x) : (far ? slab_q_far(Q0.x, Q0.y, Q0.z, qs, qb, rot, tmin, lim, t0) : slab_q(Q0.x, Q0.y, Q0.z, qs, qb, rot, tmin, lim, t0));
        const bool h1 = open_all ? box_present(Q0.w) : (far ? slab_q_far(Q0.w, Q1.x, Q1.y, qs, qb, rot, tmin, lim, t1) : slab_q(Q0.w, Q1.x, Q1.y, qs, qb, rot, tmin, lim, t1));
        if (open_all) { t0 = 0.0f; t1 = 0.0f; }
        if (h0 && h1) {
          const bool swap = t1 < t0;
          st.push(swap ? (int)Q1.z : (int)Q1.w);
          cur = swap ? (int)Q1.w : (int)Q1.z;
        } else if (h0) cur = (int)Q1.z;
        else if (h1) cur = (int)Q1.w;
        else cur = st.pop();
      }
      if (walk_trip_done(need, cur)) break;
    }

    if (!need && cur < 0 && cur > REF_MARK && cur_inst >= 0) {
      // ---- BLAS leaf: every accepted candidate is counted and, if it belongs in the row, inserted in (t, inst, prim) order
      uint32_t first, nt;
      walk_leaf(cur, first, nt);
      for (uint32_t j = 0; j < nt; j++) {
        const float4* tp = a.sc.tris + (size_t)(first + j) * 3;
        const float4 T0 = tp[0], T1 = tp[1], T2 = tp[2];
        float tt, uu, vv;
        if (!tri_test_facing(T0, T1, T2, co, cd, tmin, tmax, qword, tt, uu, vv)) continue;
        const int prim = (int)__float_as_uint(T2.y);
        const uint32_t m = count < K ? count : K;   // entries in the row
        count++;
        if (K == 0u) continue;                      // count-only
        uint32_t p = m;                             // the new entry's slot, found from the back
        if (m == K) {                               // full: it must precede the K-th entry, which falls off
          if (!hit_before(tt, cur_inst, prim, row[K - 1u])) continue;
          p = K - 1u;
        }
        while (p > 0u) {
          const HitRec e = row[p - 1u];
          if (!hit_before(tt, cur_inst, prim, e)) break;
          row[p] = e;
          p--;
        }
        HitRec h; h.t = tt; h.u = uu; h.v = vv; h.prim = prim; h.inst = cur_inst;
        row[p] = h;
        if (prune && count >= K) lim = row[K - 1u].t;
      }
      cur = st.pop();
    }
    if (!need && cur == REF_MARK) {
      // ---- leave the instance: back to world space if a TLAS node follows
      cur_inst = -1;
      cur = st.pop();
      if (cur >= 0) world_space();
    }
    if (!need && cur < 0 && cur > REF_MARK && cur_inst < 0) {
      // ---- TLAS leaf: enter the instance if the ray's mask and opacity rules let it (ray -> object space, t preserved)
      const int ii = ~cur;
      const InstanceDev* I = a.sc.inst + ii;
      uint32_t cull;
      if (query_enters(qword, I->mask, cull)) {
        qword = (qword & ~(QF_CULL_NEG | QF_CULL_POS)) | cull;
        co = xform_point(I->w2o, wo); cd = xform_vec(I->w2o, wd);
        quant_space(co, cd, I->q_lo, I->q_scale, qs, qb, rot); far = quant_far_o(co, I->q_lo, I->q_scale);
        st.push(REF_MARK);
        cur_inst = ii; cur = I->blas_root;
      } else {
        cur = st.pop();
        if (cur >= 0) world_space();
      }
    }
    if (!need && cur == REF_DONE) {
      // ---- finished: the rest of the row in rt_intersect's miss form, the count
      HitRec miss; miss.t = tmax; miss.u = 0.f; miss.v = 0.f; miss.prim = -1; miss.inst = -1;
      for (uint32_t j = count < K ? count : K; j < K; j++) row[j] = miss;
      if (a.counts) a.counts[ray] = count;
      need = true;
    }
  }
}

// rt_hit_attr of every record of the n x k rows: k_hit_attr's surface (hit_surface) and objectIndex, and k_hit_kind's facing in word 7
// with the direction of ray i / k.  A kernel of its own: the walk's register budget stays what it is.
__global__ __launch_bounds__(256) void k_query_hits_surface(SceneDev sc, const float4* __restrict__ rays, const HitRec* __restrict__ hits,
                                                            float4* __restrict__ attr, uint32_t total, uint32_t k) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  const HitRec h = hits[i];
  float4 a0 = make_float4(0.f, 0.f, 0.f, __int_as_float(-1)), a1 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (h.inst >= 0) {
    const InstanceDev* I = sc.inst + h.inst;
    const Surface S = hit_surface(sc, I, (uint32_t)h.prim, h.u, h.v);
    const float4 rd = rays[2u * (size_t)(i / k) + 1u];
    const F3 cd = xform_vec(I->w2o, mk3(rd.x, rd.y, rd.z));
    const uint32_t* ix = sc.idx + I->first_index + 3u * (uint32_t)h.prim;
    const float* vb = sc.verts + I->first_float;
    const float* p0 = vb + 6u * ix[0]; const float* p1 = vb + 6u * ix[1]; const float* p2 = vb + 6u * ix[2];
    const F3 e1 = mk3(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]), e2 = mk3(p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]);
    const float det = dot3(e1, cross3(cd, e2));
    const bool front = ((det < 0.0f) == FRONT_IS_DET_NEGATIVE) != (((I->mask >> 8) & INST_FLAG_FLIP_FACING) != 0u);
    a0 = make_float4(S.P.x, S.P.y, S.P.z, __int_as_float(I->custom_index));
    a1 = make_float4(S.N.x, S.N.y, S.N.z, __uint_as_float(front ? 0xFEu : 0xFFu));
  }
  attr[2u * (size_t)i] = a0; attr[2u * (size_t)i + 1u] = a1;
}

void launch_query_hits(const SceneDev& sc, const float4* rays, const uint32_t* words, uint32_t query_word, uint32_t n, uint32_t k, HitRec* hits,
                       float4* attr, uint32_t* counts, int32_t* ovf_stack, uint32_t* counters, const LaunchCfg& cfg, hipStream_t s) {
  HitsArgs a{};
  a.sc = sc; a.rays = rays; a.ray_words = words; a.query_word = query_word; a.n = n; a.k = k; a.hits = hits; a.counts = counts; a.ovf_stack = ovf_stack;
  launch_walk(k_query_hits, k_query_hits, a, counters, false, cfg, s);   // (no counting form)
  if (attr) {
    const uint32_t total = n * k;
    hipLaunchKernelGGL(k_query_hits_surface, dim3((total + 255u) / 256u), dim3(256), 0, s, sc, rays, (const HitRec*)hits, attr, total, k);
  }
}
