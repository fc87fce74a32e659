// kernels_ipairs.inc — included by kernels.hip after kernels_pairs.inc (product and alt translation units alike).
// rt_instance_pairs_device: the broad phase over the scene's instances (DESIGN.md §5 "Instance broad phase").  A record (rt_inst_ref, 16
// bytes: inst, against, r_max, reserved) asks which instances' canonical boxes come within the margin r_max of the canonical box of
// instance `inst`; the answer is a CSR list of rt_inst_ref records (inst, j, r_max, 0), the input of the instance-pair queries.
//
//  * k_ipairs_boxes, one thread per instance: the canonical box of the instance and a word of flags into the query workspace, 32 bytes
//    each.  The box depends on the record and on the mesh's exact bounds only (the device mesh table, found through blas_root), never
//    on a tree: the eight corners of the bounds through o2w in binary64, each rounded once, their bounds widened by 2^-13 of the
//    row-term magnitude mw of o2w over the bounds (the same quantity k_closest_scale makes from the quantisation frame);
//  * the count walk and the fill walk, one lane per record over the quantised TLAS with walk_common.inc's stack, feed and counters.
//    Box(j) may be wider than j's TLAS leaf box (mw exceeds the world coordinates when a translation cancels the mesh's own offset, and
//    the leaf's pad is 1e-5 of the world coordinates), so the node test inflates the query by a bound on every instance's widening as
//    well: 2^-13 (1 + 2^-10) of k_closest_scale's word 0.  The test at a TLAS leaf is the exact one and reads the box array only.  A
//    record with against >= 0 starts at that instance's leaf reference with nothing beneath it: the TLAS is never walked;
//  * k_list_scan_* (kernels_list.inc) between the two walks turn the counts into the n + 1 offsets;
//  * the fill walk keeps a row of at most RT_LIST_INSERT_MAX entries sorted by insertion; a longer one is written in walk order and
//    k_ipairs_sort, list_sort_body over the `against` words of the row (inst and r_max are the same in every record of a row), sorts it.

constexpr uint32_t IBOX_HAS_BOX = 0x1u;      // the instance has a canonical box: it can be a candidate
constexpr uint32_t IBOX_SOURCE = 0x2u;       // ... and it is a valid source: not void, and its mesh has an active triangle
constexpr uint32_t IBOX_MASK_SHIFT = 8;      // bits 8-15: the mask as the world-space queries see it
constexpr float IPAIR_NODE_SLACK = OB_ABS * 1.0009765625f;   // 2^-13 (1 + 2^-10): above every e_j, and the roundings of Box(j) and of the query's planes

// instance i: (lo.xyz, flags) and (hi.xyz, 0) at boxes[2 i], boxes[2 i + 1]
__global__ __launch_bounds__(256) void k_ipairs_boxes(const InstanceDev* __restrict__ inst, const TlasMeshDev* __restrict__ meshes, uint32_t n_meshes,
                                                       float4* __restrict__ boxes, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const InstanceDev* I = inst + i;
  const float* M = I->o2w;
  uint32_t flags = 0u;
  float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
  // the instance's mesh: the built mesh with triangles whose root this is (such roots are distinct)
  uint32_t mi = n_meshes;
  if (I->prim_count != 0u)
    for (uint32_t m = 0; m < n_meshes; m++)
      if (meshes[m].blas_root == I->blas_root && meshes[m].prim_count == I->prim_count && meshes[m].built != 0u) { mi = m; break; }
  if (mi < n_meshes && !(meshes[mi].lo[0] > meshes[mi].hi[0])) {
    float mlo[3], mhi[3];
    for (int k = 0; k < 3; k++) { mlo[k] = meshes[mi].lo[k]; mhi[k] = meshes[mi].hi[k]; }
    float blo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, bhi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    float mag = 0.f;
    for (int cx = 0; cx < 8; cx++) {
      const double p[3] = {(cx & 1) ? mhi[0] : mlo[0], (cx & 2) ? mhi[1] : mlo[1], (cx & 4) ? mhi[2] : mlo[2]};
      for (int r = 0; r < 3; r++) {
        const double v = (double)M[4 * r] * p[0] + (double)M[4 * r + 1] * p[1] + (double)M[4 * r + 2] * p[2] + (double)M[4 * r + 3];
        blo[r] = fminf(blo[r], (float)v); bhi[r] = fmaxf(bhi[r], (float)v);
        mag = fmaxf(mag, (float)__builtin_fabs(v));
      }
    }
    // the void rule of rt_set_instances (instance_record_state): a finite transform, the 1e-5 padded box inside INST_BOX_LIMIT
    const float pad = 1e-5f * mag + 1e-30f;
    bool live = true;
    for (int k = 0; k < 12; k++) live = live && __builtin_fabsf(M[k]) <= 3.4028234e38f;
    for (int k = 0; k < 3; k++) live = live && __builtin_fabsf(blo[k] - pad) < INST_BOX_LIMIT && __builtin_fabsf(bhi[k] + pad) < INST_BOX_LIMIT;
    // the slack: 2^-13 of the row-term magnitude over the exact bounds, unfused, left to right
    float bm[3], mw = 0.f;
    for (int k = 0; k < 3; k++) bm[k] = fmaxf(__builtin_fabsf(mlo[k]), __builtin_fabsf(mhi[k]));
    bool finite = true;   // (fmaxf drops a NaN row)
    for (int r = 0; r < 3; r++) {
      const float row = ((__builtin_fabsf(M[4 * r]) * bm[0] + __builtin_fabsf(M[4 * r + 1]) * bm[1]) + __builtin_fabsf(M[4 * r + 2]) * bm[2]) + __builtin_fabsf(M[4 * r + 3]);
      mw = fmaxf(mw, row);
      finite = finite && row <= 3.4028234e38f;
    }
    if (finite) {
      const float e = OB_ABS * mw;
      for (int k = 0; k < 3; k++) { lo[k] = blo[k] - e; hi[k] = bhi[k] + e; }
      flags = IBOX_HAS_BOX | (live ? IBOX_SOURCE : 0u);
    }
  }
  flags |= ((I->mask >> INST_WORLD_MASK_SHIFT) & 0xFFu) << IBOX_MASK_SHIFT;
  boxes[2u * i] = make_float4(lo[0], lo[1], lo[2], __uint_as_float(flags));
  boxes[2u * i + 1u] = make_float4(hi[0], hi[1], hi[2], 0.f);
}

struct IpairArgs {
  SceneDev sc;
  const int4* irefs;           // n records (rt_inst_ref)
  const float4* boxes;         // k_ipairs_boxes: two per instance
  const float* inst_scale;     // k_closest_scale: [0] the largest row-term magnitude of any instance's o2w
  uint32_t cull_mask;
  uint32_t above;              // RT_INSTANCE_PAIRS_ABOVE: only candidates above the source
  uint32_t n;
  uint32_t* counts;            // the count walk: n row lengths
  uint32_t* cursor;            // chunk cursor (zero before the launch)
  uint32_t* counters;          // the query's counter block (counting form: CNT_NODE_VISITS, CNT_TRI_TESTS)
  int32_t* ovf_stack;          // ovf_stride ints per thread of the grid
  // the fill walk only
  const unsigned long long* offsets;   // n + 1 row starts
  unsigned long long capacity; // records of pairs: a row that ends beyond it is not written
  int4* pairs;                 // the rows
  uint32_t* worklist;          // the rows left in walk order (longer than RT_LIST_INSERT_MAX), for k_ipairs_sort
  uint32_t* work_count;        // their number (zero before the launch)
};

// COUNT: the counting form (node visits, exact box tests); FILL: the rows, not their lengths
template <bool COUNT, bool FILL>
__device__ __forceinline__ void ipairs_body(const IpairArgs& a) {
  __shared__ int s_stack[4][STACK2_LDS][64];
  WalkStack st(s_stack, a.ovf_stack, a.sc.ovf_stride);
  WalkFeed feed;
  bool need = true;
  uint32_t bx = 0, count = 0, len = 0;
  F3 xlo = mk3(0, 0, 0), xhi = xlo;           // Box(inst) inflated by the margin: the exact test's
  F3 qlo = xlo, qhi = xlo;                    // ... and by the node slack: the node test's
  int src = 0, rbits = 0, skip = -1, floor_j = 0;
  int cur = REF_DONE;
  int4* row = nullptr;
  unsigned long long cnt_nodes = 0, cnt_tris = 0;
  F3 q_lo, q_scale;
  tlas_dequant(a.sc, q_lo, q_scale);

  for (;;) {
    // ---- refill: idle lanes take the next records of the wave's chunk
    const uint32_t rec = feed.take(__ballot(need), a.cursor, a.n);
    if (need && rec != WALK_NONE) {
      bx = rec;
      const int4 r = a.irefs[bx];
      const float m = __int_as_float(r.z);
      src = r.x; rbits = r.z;
      bool valid = r.x >= 0 && r.x < a.sc.n_inst && r.y >= -1 && r.y < a.sc.n_inst && m >= 0.0f;
      if (valid) {
        const float4 A = a.boxes[2u * (uint32_t)r.x], B = a.boxes[2u * (uint32_t)r.x + 1u];
        valid = (__float_as_uint(A.w) & IBOX_SOURCE) != 0u;
        xlo = mk3(A.x - m, A.y - m, A.z - m); xhi = mk3(B.x + m, B.y + m, B.z + m);
        const float E = IPAIR_NODE_SLACK * a.inst_scale[0];
        qlo = mk3(xlo.x - E, xlo.y - E, xlo.z - E); qhi = mk3(xhi.x + E, xhi.y + E, xhi.z + E);
      }
      skip = r.y < 0 ? r.x : -1;
      floor_j = a.above ? r.x + 1 : 0;   // (r.x < n_inst: no overflow; an invalid record never looks)
      count = 0;
      st.reset(); cur = valid ? a.sc.tlas_root : REF_DONE;
      if (valid && r.y >= 0) cur = ~r.y;
      if (FILL) {   // the row the count walk measured: nothing to do for an empty one or one that ends beyond the capacity
        const unsigned long long o0 = a.offsets[bx], o1 = a.offsets[bx + 1u];
        len = o1 > a.capacity ? 0u : (uint32_t)(o1 - o0);
        if (len == 0u) cur = REF_DONE;
        row = a.pairs + o0;
      }
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

    if (!need && cur < 0 && cur > REF_MARK) {
      // ---- TLAS leaf: the exact test against the candidate's canonical box, closed
      const int j = ~cur;
      const float4 A = a.boxes[2u * (uint32_t)j], B = a.boxes[2u * (uint32_t)j + 1u];
      const uint32_t fl = __float_as_uint(A.w);
      if (COUNT) cnt_tris++;
      const bool cand = (fl & IBOX_HAS_BOX) != 0u && ((fl >> IBOX_MASK_SHIFT) & a.cull_mask & 0xFFu) != 0u && j != skip && j >= floor_j &&
                        !(xlo.x > B.x) && !(xhi.x < A.x) && !(xlo.y > B.y) && !(xhi.y < A.y) && !(xlo.z > B.z) && !(xhi.z < A.z);
      if (cand) {
        if (FILL && count < len) {   // every candidate has its place: a short row by insertion on `against`, a long one in walk order
          uint32_t p = count;
          row[p] = make_int4(src, j, rbits, 0);
          if (len <= (uint32_t)RT_LIST_INSERT_MAX) {
            int32_t* w = reinterpret_cast<int32_t*>(row) + 1;   // the `against` words, four apart
            while (p > 0u) {
              const int32_t o = w[4u * (p - 1u)];
              if (!(j < o)) break;
              w[4u * p] = o;
              p--;
            }
            w[4u * p] = j;
          }
        }
        count++;
      }
      cur = st.pop();
    }
    if (!need && cur == REF_DONE) {
      // ---- finished: the row's length, or a long row to k_ipairs_sort
      if (FILL) {
        if (len > (uint32_t)RT_LIST_INSERT_MAX) a.worklist[atomicAdd(a.work_count, 1u)] = bx;
      } else a.counts[bx] = count;
      need = true;
    }
  }
  if (COUNT) walk_flush_counters(a.counters, cnt_nodes, cnt_tris);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_ipairs_size(IpairArgs a) { ipairs_body<false, false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_ipairs_size_count(IpairArgs a) { ipairs_body<true, false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_ipairs_fill(IpairArgs a) { ipairs_body<false, true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_ipairs_fill_count(IpairArgs a) { ipairs_body<true, true>(a); }

// ---- sort: the `against` words of a row, 16 bytes apart; non-negative and distinct within a row
struct ListAgainst {
  typedef int4 Rec;
  typedef uint32_t Key;
  __device__ __forceinline__ static Key key(const int4* rows, size_t i) { return (uint32_t)reinterpret_cast<const int32_t*>(rows + i)[1]; }
  __device__ __forceinline__ static void put(int4* rows, size_t i, Key key) { reinterpret_cast<int32_t*>(rows + i)[1] = (int32_t)key; }
};
struct IpairSortArgs {
  int4* pairs;
  const unsigned long long* offsets;
  const uint32_t* worklist;
  const uint32_t* work_count;
};
__global__ __launch_bounds__(256) void k_ipairs_sort(IpairSortArgs a) {
  __shared__ uint32_t s_keys[LIST_TILE];
  list_sort_body<ListAgainst>(a.pairs, a.offsets, a.worklist, a.work_count, s_keys);
}

// ---- launch

void launch_ipairs_boxes(const SceneDev& sc, const void* mesh_table, uint32_t n_meshes, float4* boxes, hipStream_t s) {
  if (sc.n_inst > 0)
    hipLaunchKernelGGL(k_ipairs_boxes, dim3(((uint32_t)sc.n_inst + 255u) / 256u), dim3(256), 0, s, sc.inst, (const TlasMeshDev*)mesh_table, n_meshes, boxes, (uint32_t)sc.n_inst);
}

static IpairArgs ipair_args(const SceneDev& sc, const void* irefs, const float4* boxes, const float* inst_scale, uint32_t cull_mask, bool above, uint32_t n,
                            int32_t* ovf_stack, uint32_t* counters) {
  IpairArgs a{};
  a.sc = sc; a.irefs = (const int4*)irefs; a.boxes = boxes; a.inst_scale = inst_scale; a.cull_mask = cull_mask; a.above = above ? 1u : 0u; a.n = n;
  a.counters = counters; a.ovf_stack = ovf_stack;
  return a;
}

void launch_ipairs_size(const SceneDev& sc, const void* irefs, const float4* boxes, const float* inst_scale, uint32_t cull_mask, bool above, uint32_t* counts, uint32_t n,
                        int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s) {
  IpairArgs a = ipair_args(sc, irefs, boxes, inst_scale, cull_mask, above, n, ovf_stack, counters);
  a.counts = counts;
  launch_walk(k_ipairs_size, k_ipairs_size_count, a, counters, counting, cfg, s);
}

void launch_ipairs_fill(const SceneDev& sc, const void* irefs, const float4* boxes, const float* inst_scale, uint32_t cull_mask, bool above,
                        const unsigned long long* offsets, void* pairs, uint64_t capacity, uint32_t* work, uint32_t n, int32_t* ovf_stack, uint32_t* counters,
                        bool counting, const LaunchCfg& cfg, hipStream_t s) {
  IpairArgs a = ipair_args(sc, irefs, boxes, inst_scale, cull_mask, above, n, ovf_stack, counters);
  a.offsets = offsets; a.capacity = capacity; a.pairs = (int4*)pairs; a.work_count = work; a.worklist = work + 1;
  hipMemsetAsync(work, 0, sizeof(uint32_t), s);
  launch_walk(k_ipairs_fill, k_ipairs_fill_count, a, counters, counting, cfg, s);
  IpairSortArgs t{(int4*)pairs, offsets, work + 1, work};
  hipLaunchKernelGGL(k_ipairs_sort, dim3(min((uint32_t)cfg.trace_blocks, n)), dim3(256), 0, s, t);
}
