// kernels_inside.inc — included by kernels.hip (product and alt translation units alike).
// rt_point_inside_device / rt_signed_distance_device: is a point inside the scene's surfaces?  For each point the crossings of the
// rays (p, tmin 0, D_k, tmax +inf) along a fixed table of directions are counted with the arithmetic of rt_intersect_device_hits'
// count-only query (query word 0 | cull_mask << 24), and the majority of the parities decides (DESIGN.md §5 "Inside / outside").
// A record-level walk of its own (walk_common.inc: the stack, the chunk feed, the trip exit, the counters); no existing kernel changes.
//
//  * one lane per point: the lane walks direction 0, and while the vote is undecided it restarts at the TLAS root with the next
//    direction of the table.  The early stop costs nothing, no lane waits for another lane's vote, and the ray exists in registers
//    only: nothing ray-sized touches memory;
//  * the far-ray logic always on, REF_MARK leaving an instance: k_query_hits';
//  * no rows, no per-ray words, no flags: an instance is entered when (mask & cull_mask) != 0 (what query_enters decides for the
//    word 0 | cull_mask << 24) and a leaf runs tri_test_facing without a facing cull over (0, +inf), so the counts are
//    k_query_hits' bit for bit.

struct InsideArgs {
  SceneDev sc;
  const float4* points;        // n points, 16 bytes each: (x, y, z, ignored)
  uint32_t cull_mask;
  uint32_t n_dirs;             // 1, 3 or 5
  uint32_t n;
  uint32_t* words;             // n vote words
  uint32_t* counts;            // n * n_dirs crossing counts, point-major, or null (then the vote stops early)
  uint32_t* cursor;            // chunk cursor (zero before the launch)
  uint32_t* counters;          // the query's counter block (counting)
  int32_t* ovf_stack;          // ovf_stride ints per thread of the grid
};

// the direction table of include/rt_api.h (RT_INSIDE_DIRS): used as given, not normalised
__device__ __forceinline__ F3 inside_dir(uint32_t k) {
  constexpr float T[RT_INSIDE_MAX_DIRS][3] = RT_INSIDE_DIRS;
  return mk3(k == 0u ? T[0][0] : k == 1u ? T[1][0] : k == 2u ? T[2][0] : k == 3u ? T[3][0] : T[4][0],
             k == 0u ? T[0][1] : k == 1u ? T[1][1] : k == 2u ? T[2][1] : k == 3u ? T[3][1] : T[4][1],
             k == 0u ? T[0][2] : k == 1u ? T[1][2] : k == 2u ? T[2][2] : k == 3u ? T[3][2] : T[4][2]);
}

template <bool COUNT>
__device__ __forceinline__ void inside_body(const InsideArgs& a) {
  __shared__ int s_stack[4][STACK2_LDS][64];
  WalkStack st(s_stack, a.ovf_stack, a.sc.ovf_stride);
  WalkFeed feed;
  const uint32_t n_dirs = a.n_dirs, half = a.n_dirs >> 1;
  const bool all_dirs = a.counts != nullptr;
  const float tmin = 0.0f, tmax = __builtin_inff();

  // per-lane state: the point, the direction being walked and the votes so far
  bool need = true;
  uint32_t pt = 0, count = 0, dir = 0, odd = 0;
  F3 wo = mk3(0, 0, 0), wd = mk3(0, 0, 1), co = wo, cd = wd, qs = mk3(1, 1, 1), qb = mk3(0, 0, 0);
  uint3 rot = make_uint3(0u, 0u, 0u);
  bool far = false;
  int cur = REF_DONE, cur_inst = -1;
  unsigned long long cnt_nodes = 0, cnt_tris = 0;

  auto world_space = [&]() {
    quant_space(wo, wd, a.sc.tlas_q_lo, a.sc.tlas_q_scale, qs, qb, rot); far = quant_far_o(wo, a.sc.tlas_q_lo, a.sc.tlas_q_scale);
  };
  // the ray of direction `dir` from the lane's point, at the TLAS root
  auto start_dir = [&]() {
    wd = inside_dir(dir);
    co = wo; cd = wd;
    world_space();
    cur_inst = -1; count = 0;
    st.reset(); cur = a.sc.tlas_root;
  };

  for (;;) {
    // ---- refill: idle lanes take the next points of the wave's chunk
    const uint32_t rec = feed.take(__ballot(need), a.cursor, a.n);
    if (need && rec != WALK_NONE) {
      pt = rec;
      const float4 r = ld_stream(&a.points[pt]);
      wo = mk3(r.x, r.y, r.z);
      dir = 0u; odd = 0u;
      if (finite_bits(r.x) && finite_bits(r.y) && finite_bits(r.z)) {
        start_dir();
        need = false;
      } else {
        // a point with a non-finite coordinate: word 0, counts 0; the lane stays idle and takes another point next trip
        a.words[pt] = 0u;
        if (all_dirs) for (uint32_t k = 0; k < n_dirs; k++) a.counts[(size_t)pt * n_dirs + k] = 0u;
      }
    }
    if (__ballot(!need) == 0) {
      if (feed.drained) break;   // every lane idle and the points used up
      continue;                  // (a chunk of invalid points only: take the next one)
    }

    // ---- interior nodes: every lane at one takes a visit; the trip repeats while most live lanes are interior
    for (;;) {
      if (cur >= 0) {
        uint4 Q0, Q1;
        walk_node(a.sc, cur, Q0, Q1);
        if (COUNT) cnt_nodes++;
        float t0, t1;
        const bool open_all = far && cur_inst < 0;   // (a far ray in world space: the TLAS does not cull, as in k_query_hits)
        const bool h0 = open_all ? box_present(Q0.x) : (far ? slab_q_far(Q0.x, Q0.y, Q0.z, qs, qb, rot, tmin, tmax, t0) : slab_q(Q0.x, Q0.y, Q0.z, qs, qb, rot, tmin, tmax, t0));
        const bool h1 = open_all ? box_present(Q0.w) : (far ? slab_q_far(Q0.w, Q1.x, Q1.y, qs, qb, rot, tmin, tmax, t1) : slab_q(Q0.w, Q1.x, Q1.y, qs, qb, rot, tmin, tmax, t1));
        if (h0 && h1) {
          st.push((int)Q1.w);   // (every candidate counts: no order among the children)
          cur = (int)Q1.z;
        } else if (h0) cur = (int)Q1.z;
        else if (h1) cur = (int)Q1.w;
        else cur = st.pop();
      }
      if (walk_trip_done(need, cur)) break;
    }

    if (!need && cur < 0 && cur > REF_MARK && cur_inst >= 0) {
      // ---- BLAS leaf: every accepted candidate is a crossing
      uint32_t first, nt;
      walk_leaf(cur, first, nt);
      for (uint32_t j = 0; j < nt; j++) {
        const float4* tp = a.sc.tris + (size_t)(first + j) * 3;
        const float4 T0 = tp[0], T1 = tp[1], T2 = tp[2];
        if (COUNT) cnt_tris++;
        float tt, uu, vv;
        if (tri_test_facing(T0, T1, T2, co, cd, tmin, tmax, 0u, tt, uu, vv)) count++;
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
      // ---- TLAS leaf: enter the instance if the call's mask lets it (ray -> object space, t preserved)
      const int ii = ~cur;
      const InstanceDev* I = a.sc.inst + ii;
      if ((I->mask & a.cull_mask & 0xFFu) != 0u) {
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
      // ---- a direction is finished: its vote; the word once odd or even holds the majority (or, with counts, after every direction)
      if (all_dirs) a.counts[(size_t)pt * n_dirs + dir] = count;
      odd += count & 1u;
      dir++;
      const bool decided = odd > half || dir - odd > half;
      if (dir == n_dirs || (decided && !all_dirs)) {
        a.words[pt] = (odd > half ? 1u : 0u) | (odd << 8) | (dir << 16);
        need = true;
      } else start_dir();
    }
  }
  if (COUNT) walk_flush_counters(a.counters, cnt_nodes, cnt_tris);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_HITS_WAVES_PER_EU))) void k_point_inside(InsideArgs a) { inside_body<false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_HITS_WAVES_PER_EU))) void k_point_inside_count(InsideArgs a) { inside_body<true>(a); }

// rt_signed_distance_device: the sign bit of a closest-point record's t is set where bit 0 of the point's vote word is set (a miss
// record included: -r_max; t = 0 becomes -0.0).  A record that was not a valid closest-point query (r_max negative or NaN; a non-finite
// coordinate has word 0) keeps its miss form.
__global__ __launch_bounds__(256) void k_sign_distance(const float4* __restrict__ points, const uint32_t* __restrict__ words, HitRec* __restrict__ hits, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  if ((words[i] & 1u) == 0u) return;
  if (!(points[i].w >= 0.0f)) return;
  uint32_t* const t = reinterpret_cast<uint32_t*>(&hits[i].t);
  *t |= 0x80000000u;
}

void launch_point_inside(const SceneDev& sc, const float4* points, uint32_t cull_mask, uint32_t n_dirs, uint32_t* words, uint32_t* counts, uint32_t n,
                         int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s) {
  InsideArgs a{};
  a.sc = sc; a.points = points; a.cull_mask = cull_mask; a.n_dirs = n_dirs; a.n = n; a.words = words; a.counts = counts; a.counters = counters; a.ovf_stack = ovf_stack;
  launch_walk(k_point_inside, k_point_inside_count, a, counters, counting, cfg, s);
}

void launch_sign_distance(const float4* points, const uint32_t* words, HitRec* hits, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_sign_distance, dim3((n + 255u) / 256u), dim3(256), 0, s, points, words, hits, n);
}
