// kernels_pairs.inc — included by kernels.hip after kernels_list.inc (product and alt translation units alike).
// rt_closest_instances_device, rt_overlap_instances_device: the two by-reference triangle queries asked per pair of bodies.  A record
// (rt_inst_ref, 16 bytes: inst, against, r_max, reserved) stands for every triangle of instance `inst` as rt_tri_ref (inst, p, against,
// r_max) names it, and the answer is the reduction of those per-triangle answers (DESIGN.md §5 "Instance pairs").
//
//  * k_pairs_plan, one thread per record: the record's work items (the triangle count of the source's mesh, 0 for an invalid record; inst,
//    then against, and only then sc.inst[inst], as k_refs_expand checks a reference) and the start values of what the walk reduces into;
//  * k_list_scan_* (kernels_list.inc) turn the counts into n + 1 uint64 offsets; their last, the number of items, stays on the device;
//  * the walks are the PAIRS instantiations of nearest_body and overlap_body (walk_nearest.inc, walk_overlap.inc): a lane's work item w is
//    source triangle p = w - offsets[r] of the record r a binary search of the offsets finds, its world image made at refill by
//    refs_world_triangle (kernels_refs.inc), and the start node and own-instance rule are those of the by-reference walks;
//      - nearest: the lanes of a record share one bound, the record's key (d2 bits << 32 | p, a 64-bit atomic minimum).  A lane prunes with
//        the smaller of its own best d2 and the key's; it publishes after a leaf that gave it a d2 no larger than that bound.  A subtree is
//        skipped only when its deflated bound exceeds the bound (ties arrive), so every source triangle that attains the record's minimum
//        computes its canonical d2 and publishes it; the others publish larger keys or none;
//      - overlap: count only; a lane adds its count to the record's 64-bit sum and offers p to the record's first-p word; with `any` the
//        sum word is the record's flag, set at the first candidate and read at refill and at every leaf by the record's other items;
//  * k_pairs_refs, one thread per record, writes the rt_tri_ref of the winning source triangle (an invalid reference when there is none),
//    over which the by-reference calls then make the answer: the bytes are theirs by construction;
//  * k_pairs_first, one thread per record: (p, inst, prim, 0) from the first-p word and the capped by-reference call's row of one.

constexpr uint32_t PAIR_NONE = 0xFFFFFFFFu;   // no source primitive (a call has fewer than 0xFFFFFF00 work items)

// the record of work item w: offsets[r] <= w < offsets[r + 1] (offsets[0] == 0 <= w < offsets[n]; records without items are passed over)
__device__ __forceinline__ uint32_t pair_record(const unsigned long long* offsets, uint32_t n, uint32_t w) {
  uint32_t lo = 0u, hi = n;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (offsets[mid] <= (unsigned long long)w) lo = mid; else hi = mid;
  }
  return lo;
}

// PLAN_NEAREST: keys; PLAN_OVERLAP: sums and first_p (optional)
template <bool NEAREST>
__global__ __launch_bounds__(256) void k_pairs_plan(SceneDev sc, const int4* __restrict__ irefs, uint32_t n, uint32_t* __restrict__ items,
                                                     unsigned long long* __restrict__ keys, unsigned long long* __restrict__ sums, uint32_t* __restrict__ first_p) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int4 r = irefs[i];
  const int inst = r.x, against = r.y;
  const float r_max = __int_as_float(r.z);
  uint32_t count = 0u;
  if (inst >= 0 && inst < sc.n_inst && against >= -1 && against < sc.n_inst && (!NEAREST || r_max >= 0.0f)) count = sc.inst[inst].prim_count;
  items[i] = count;
  if (NEAREST) keys[i] = ((unsigned long long)__float_as_uint(r_max * r_max) << 32) | (unsigned long long)PAIR_NONE;
  else {
    sums[i] = 0ull;
    if (first_p) first_p[i] = PAIR_NONE;
  }
}

// ---- the shapes: a source triangle of a record as the triangle shapes' query

struct PairNearest : NearestTriangle {
  uint32_t r = 0u, p = 0u;                    // the record and the source primitive
  unsigned long long seen = 0ull;             // the record's key as last loaded, or what this lane published since
  __device__ __forceinline__ bool load(const NearestArgs& a, uint32_t w, float& r_max, float& pmag, int& against) {
    r = pair_record(a.offsets, a.n, w);
    p = w - (uint32_t)a.offsets[r];
    const int4 ir = a.irefs[r];   // (k_pairs_plan gave an invalid record no items: inst and against are in range)
    against = ir.y; r_max = __int_as_float(ir.z);
    w0 = mk3(0, 0, 0); w1 = w0; w2 = w0;
    const bool made = refs_world_triangle(a.sc, a.sc.inst + ir.x, (int)p, a.n_vert_floats, w0, w1, w2);
    pmag = fmaxf(fmaxf(fmaxf(fmaxf(__builtin_fabsf(w0.x), __builtin_fabsf(w0.y)), __builtin_fabsf(w0.z)),
                       fmaxf(fmaxf(__builtin_fabsf(w1.x), __builtin_fabsf(w1.y)), __builtin_fabsf(w1.z))),
                 fmaxf(fmaxf(__builtin_fabsf(w2.x), __builtin_fabsf(w2.y)), __builtin_fabsf(w2.z)));
    return made;
  }
  __device__ __forceinline__ bool own(const NearestArgs& a, uint32_t, int ii) const {
    const int4 ir = a.irefs[r];
    return ir.y < 0 && ii == ir.x;
  }
  // the smallest d2 any lane of the record has published: neither hoisted nor cached
  __device__ __forceinline__ float shared(const NearestArgs& a) {
    const unsigned long long k = __hip_atomic_load(a.keys + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    seen = k;   // (the key only falls, and this lane's own publications are in it)
    return __uint_as_float((uint32_t)(k >> 32));
  }
  // d2 (never negative, never NaN: unsigned order of the bits is float order) is this lane's: into the key unless it could not lower it
  __device__ __forceinline__ void publish(const NearestArgs& a, float d2) {
    const unsigned long long mine = ((unsigned long long)__float_as_uint(d2 + 0.0f) << 32) | (unsigned long long)p;
    if (mine < seen) {
      __hip_atomic_fetch_min(a.keys + r, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      seen = mine;
    }
  }
  __device__ __forceinline__ static void store(const NearestArgs&, uint32_t, Params) {}
};

struct PairOverlap {
  struct Item { F3 P0, P1, P2; uint32_t r, p; };
  __device__ __forceinline__ static bool load(const OverlapArgs& a, uint32_t w, Item& it, F3& wlo, F3& whi, float& mag, int& against) {
    it.r = pair_record(a.offsets, a.n, w);
    it.p = w - (uint32_t)a.offsets[it.r];
    const int4 ir = a.irefs[it.r];   // (k_pairs_plan gave an invalid record no items: inst and against are in range)
    against = ir.y;
    it.P0 = mk3(0, 0, 0); it.P1 = it.P0; it.P2 = it.P0;
    const bool made = refs_world_triangle(a.sc, a.sc.inst + ir.x, (int)it.p, a.n_vert_floats, it.P0, it.P1, it.P2);
    wlo = mk3(fminf(fminf(it.P0.x, it.P1.x), it.P2.x), fminf(fminf(it.P0.y, it.P1.y), it.P2.y), fminf(fminf(it.P0.z, it.P1.z), it.P2.z));
    whi = mk3(fmaxf(fmaxf(it.P0.x, it.P1.x), it.P2.x), fmaxf(fmaxf(it.P0.y, it.P1.y), it.P2.y), fmaxf(fmaxf(it.P0.z, it.P1.z), it.P2.z));
    mag = fmaxf(fmaxf(fmaxf(__builtin_fabsf(wlo.x), __builtin_fabsf(wlo.y)), __builtin_fabsf(wlo.z)),
                fmaxf(fmaxf(__builtin_fabsf(whi.x), __builtin_fabsf(whi.y)), __builtin_fabsf(whi.z)));
    return made;
  }
  struct Leaf {
    const Item& it;
    __device__ __forceinline__ Leaf(const OverlapArgs&, uint32_t, const Item& item) : it(item) {}
    __device__ __forceinline__ bool touches(F3 wlo, F3 whi, F3 A, F3 ab, F3 ac) const { return collide_tri(wlo, whi, it.P0, it.P1, it.P2, A, ab, ac); }
  };
  __device__ __forceinline__ static bool own(const OverlapArgs& a, const Item& it, int ii) {
    const int4 ir = a.irefs[it.r];
    return ir.y < 0 && ii == ir.x;
  }
  // any: an item of the record has found a contact
  __device__ __forceinline__ static bool ended(const OverlapArgs& a, const Item& it) {
    return a.any != 0u && __hip_atomic_load(a.sums + it.r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull;
  }
  // an item with candidates: into the record's sum and first-p word; any: the flag
  __device__ __forceinline__ static void finish(const OverlapArgs& a, const Item& it, uint32_t count) {
    if (a.any) { __hip_atomic_store(a.sums + it.r, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); return; }
    __hip_atomic_fetch_add(a.sums + it.r, (unsigned long long)count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (a.first_p) __hip_atomic_fetch_min(a.first_p + it.r, it.p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_TRIANGLE_WAVES_PER_EU))) void k_pairs_nearest(NearestArgs a) { nearest_body<PairNearest, false, true, true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_TRIANGLE_WAVES_PER_EU))) void k_pairs_nearest_count(NearestArgs a) { nearest_body<PairNearest, true, true, true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_pairs_collide(OverlapArgs a) { overlap_body<PairOverlap, false, true, false, true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_pairs_collide_count(OverlapArgs a) { overlap_body<PairOverlap, true, true, false, true>(a); }

// ---- finish

// The reference of every record's winning source triangle from `word` (nearest: the low word of the key, stride 2; overlap: the first-p
// word, stride 1): (inst, p, against, r_max), or (-1, -1, -1, r_max) when there is none, which the by-reference calls answer in the miss
// form with the radius as given.  src_prims (optional): p, or -1.  keep_radius: the overlap query's references carry a radius of 0.
__global__ __launch_bounds__(256) void k_pairs_refs(const int4* __restrict__ irefs, const uint32_t* __restrict__ word, uint32_t stride, uint32_t n, uint32_t keep_radius,
                                                     int4* __restrict__ refs, int32_t* __restrict__ src_prims) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int4 r = irefs[i];
  const uint32_t p = word[(size_t)i * stride];
  const int radius = keep_radius ? r.z : 0;
  refs[i] = p != PAIR_NONE ? make_int4(r.x, (int)p, r.y, radius) : make_int4(-1, -1, -1, radius);
  if (src_prims) src_prims[i] = (int32_t)p;   // (PAIR_NONE: -1)
}

// rt_overlap_instances_device's d_first4: (p, inst, prim, 0), the row of one of the capped by-reference call behind the first-p word
__global__ __launch_bounds__(256) void k_pairs_first(const uint32_t* __restrict__ first_p, const IdRec* __restrict__ ids, uint32_t n, int32_t* __restrict__ first4) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const IdRec id = ids[i];
  int32_t* o = first4 + 4u * (size_t)i;
  o[0] = (int32_t)first_p[i]; o[1] = id.inst; o[2] = id.prim; o[3] = 0;
}

// ---- launch

void launch_pairs_plan(const SceneDev& sc, const void* irefs, uint32_t n, bool nearest, uint32_t* items, unsigned long long* sums_scratch, unsigned long long* offsets,
                       unsigned long long* keys, unsigned long long* sums, uint32_t* first_p, hipStream_t s) {
  const dim3 g((n + 255u) / 256u), b(256);
  if (nearest) hipLaunchKernelGGL((k_pairs_plan<true>), g, b, 0, s, sc, (const int4*)irefs, n, items, keys, sums, first_p);
  else hipLaunchKernelGGL((k_pairs_plan<false>), g, b, 0, s, sc, (const int4*)irefs, n, items, keys, sums, first_p);
  launch_list_scan(items, n, sums_scratch, offsets, s);
}

// the grid of a walk over at most max_items work items, whose number the device holds
static uint32_t pairs_blocks(uint64_t max_items, const LaunchCfg& cfg) {
  const uint64_t want = (max_items + 255u) / 256u;
  return want < (uint64_t)cfg.trace_blocks ? (uint32_t)(want ? want : 1u) : (uint32_t)cfg.trace_blocks;
}

void launch_pairs_nearest(const SceneDev& sc, const void* irefs, const unsigned long long* offsets, unsigned long long* keys, uint32_t cull_mask, const float* inst_scale,
                          uint32_t n, uint64_t max_items, uint64_t n_vert_floats, int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s) {
  NearestArgs a{};
  a.sc = sc; a.inst_scale = inst_scale; a.cull_mask = cull_mask; a.n = n; a.counters = counters; a.ovf_stack = ovf_stack;
  a.irefs = (const int4*)irefs; a.offsets = offsets; a.keys = keys;
  a.n_vert_floats = (uint32_t)(n_vert_floats < 0xFFFFFFFFull ? n_vert_floats : 0xFFFFFFFFull);
  hipLaunchKernelGGL(k_query_init, dim3(1), dim3(64), 0, s, counters, n);
  a.cursor = counters + cnt_work(0, 0);
  hipLaunchKernelGGL(counting ? k_pairs_nearest_count : k_pairs_nearest, dim3(pairs_blocks(max_items, cfg)), dim3(256), 0, s, a);
}

void launch_pairs_collide(const SceneDev& sc, const void* irefs, const unsigned long long* offsets, unsigned long long* sums, uint32_t* first_p, bool any, uint32_t cull_mask,
                          const float* inst_scale, uint32_t n, uint64_t max_items, uint64_t n_vert_floats, int32_t* ovf_stack, uint32_t* counters, bool counting,
                          const LaunchCfg& cfg, hipStream_t s) {
  OverlapArgs a = overlap_args(sc, nullptr, cull_mask, inst_scale, nullptr, n, ovf_stack, counters);
  a.any = any ? 1u : 0u; a.offsets = offsets; a.irefs = (const int4*)irefs; a.sums = sums; a.first_p = first_p;
  a.n_vert_floats = (uint32_t)(n_vert_floats < 0xFFFFFFFFull ? n_vert_floats : 0xFFFFFFFFull);
  hipLaunchKernelGGL(k_query_init, dim3(1), dim3(64), 0, s, counters, n);
  a.cursor = counters + cnt_work(0, 0);
  hipLaunchKernelGGL(counting ? k_pairs_collide_count : k_pairs_collide, dim3(pairs_blocks(max_items, cfg)), dim3(256), 0, s, a);
}

void launch_pairs_refs(const void* irefs, const uint32_t* word, uint32_t stride, uint32_t n, bool keep_radius, void* refs, int32_t* src_prims, hipStream_t s) {
  hipLaunchKernelGGL(k_pairs_refs, dim3((n + 255u) / 256u), dim3(256), 0, s, (const int4*)irefs, word, stride, n, keep_radius ? 1u : 0u, (int4*)refs, src_prims);
}

void launch_pairs_first(const uint32_t* first_p, const void* ids, uint32_t n, void* first4, hipStream_t s) {
  hipLaunchKernelGGL(k_pairs_first, dim3((n + 255u) / 256u), dim3(256), 0, s, first_p, (const IdRec*)ids, n, (int32_t*)first4);
}
