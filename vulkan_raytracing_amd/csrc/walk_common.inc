// walk_common.inc — included by kernels.hip before kernels_hits.inc (product and alt translation units alike).
// The skeleton of a record-level walk: one lane per record, the quantised BVH2 of the TLAS and, inside an instance, of its BLAS.  What
// every such walk does the same way lives here.  On top of it:
//  * k_query_hits, k_closest_hits, k_sweep_spheres and k_point_inside each have a body in their own file: node test, child order, leaf
//    body, instance entry and exit, finish step, args struct and register budget;
//  * the nearest-pair walks (k_closest_point, k_closest_segment, k_closest_triangle, k_refs_nearest) share the body, args struct and
//    launch of walk_nearest.inc, the overlap walks (k_overlap_boxes, k_collide_triangles, k_refs_collide, k_list_*) those of
//    walk_overlap.inc.  What stays in such a walk's own file is its shape: the record and its validity, the form the node test reads,
//    the node test (nearest), the canonical leaf test, the result words beside the hit record, and the register budget switch.
//  * k_ipairs_size and k_ipairs_fill (kernels_ipairs.inc) walk the TLAS only, a record's box against the instances' boxes.
// The frame kernels and k_trace have a stack of their own (the fast_step row) and use none of this.

// The per-lane stack: STACK2_LDS entries in the block's LDS array (entry e at stk[e * 64]), deeper ones in the query's spill area
// (ovf_stride ints per thread of the grid).  The spill words are volatile: never merged with the LDS access into a flat one.
struct WalkStack {
  int* stk;
  int32_t* ovf;
  int sp;
  __device__ __forceinline__ WalkStack(int (&lds)[4][STACK2_LDS][64], int32_t* ovf_stack, uint32_t ovf_stride)
      : stk(&lds[threadIdx.x >> 6][0][threadIdx.x & 63u]), ovf(ovf_stack + (size_t)(blockIdx.x * 256u + threadIdx.x) * ovf_stride), sp(0) {}
  __device__ __forceinline__ void reset() { stk[0] = REF_DONE; sp = 1; }   // (the sentinel ends the record)
  __device__ __forceinline__ void push(int v) {
    if (sp < STACK2_LDS) stk[sp * 64] = v;
    else *reinterpret_cast<volatile int32_t*>(ovf + (sp - STACK2_LDS)) = v;
    sp++;
  }
  __device__ __forceinline__ int pop() {
    sp--;
    if (sp < STACK2_LDS) return stk[sp * 64];
    return *reinterpret_cast<volatile int32_t*>(ovf + (sp - STACK2_LDS));
  }
};

// The wave-uniform work distribution: a wave takes 64-record chunks from one cursor of the query's counter block (zero before the
// launch), and a lane that finishes takes the next record of the wave's chunk (ballot + prefix rank), so lanes stay busy.
constexpr uint32_t WALK_NONE = 0xFFFFFFFFu;   // (a call has fewer than 0xFFFFFF00 records)
struct WalkFeed {
  uint32_t chunk_next = 0, chunk_end = 0;
  bool drained = false;   // the cursor is past the last record
  // Once per outer trip, by every lane of the wave; need_mask: the ballot of the idle lanes.  Returns the record an idle lane takes, or
  // WALK_NONE when the chunk (or the query) has none left for it; a busy lane ignores the value.  A new chunk is fetched when the
  // current one is used up.  (The ballot and one returned value, not the lane's own flag or a flag beside the index: either form
  // costs the walks registers, profiles/query_walk_refactor.txt.)
  __device__ __forceinline__ uint32_t take(uint64_t need_mask, uint32_t* cursor, uint32_t n) {
    uint32_t rec = WALK_NONE;
    if (need_mask != 0 && !drained) {
      if (chunk_next == chunk_end) {
        uint32_t c = 0;
        if ((threadIdx.x & 63u) == 0) c = atomicAdd(cursor, 1u);
        c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
        const uint64_t b = (uint64_t)c * 64u;
        if (b >= n) drained = true;
        else { chunk_next = (uint32_t)b; chunk_end = (uint32_t)min((uint64_t)n, b + 64u); }
      }
      if (!drained) {
        const uint32_t rank = prefix_rank(need_mask), avail = chunk_end - chunk_next;
        if (rank < avail) rec = chunk_next + rank;
        const uint32_t n_need = (uint32_t)__builtin_popcountll(need_mask);
        chunk_next += n_need < avail ? n_need : avail;
      }
    }
    return rec;
  }
};

// the end of an interior trip: every lane at an interior node has taken a visit; the trip repeats while most live lanes are interior
__device__ __forceinline__ bool walk_trip_done(bool need, int cur) {
  const uint32_t live = 64u - (uint32_t)__builtin_popcountll(__ballot(need));
  const uint32_t n_int = (uint32_t)__builtin_popcountll(__ballot(cur >= 0));
  return n_int == 0 || n_int * 8u < live * 5u;
}

// the two 16-byte halves of interior node `cur` (BvhNodeQ): child 0's box in Q0.xyz, child 1's in (Q0.w, Q1.x, Q1.y), the children in Q1.zw
__device__ __forceinline__ void walk_node(const SceneDev& sc, int cur, uint4& Q0, uint4& Q1) {
  const uint4* np = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(sc.blas_nodes) + ((uint32_t)cur << 5));
  Q0 = np[0]; Q1 = np[1];
}

// the packets of leaf reference `cur` (negative, above REF_MARK): nt of them from `first`
__device__ __forceinline__ void walk_leaf(int cur, uint32_t& first, uint32_t& nt) {
  const uint32_t ref = (uint32_t)(~cur);
  first = ref >> 3; nt = (ref & 7u) + 1u;
}

// a missing child is an inverted box (lo above hi in the x word)
__device__ __forceinline__ bool box_present(uint32_t wx) { return (wx & 0xFFFFu) <= (wx >> 16); }

// the planes of the quantised box (wx, wy, wz) of a tree with dequantisation (q_lo, q_scale)
__device__ __forceinline__ void box_planes(uint32_t wx, uint32_t wy, uint32_t wz, F3 q_lo, F3 q_scale, F3& lo, F3& hi) {
  lo.x = __builtin_fmaf((float)(wx & 0xFFFFu), q_scale.x, q_lo.x); hi.x = __builtin_fmaf((float)(wx >> 16), q_scale.x, q_lo.x);
  lo.y = __builtin_fmaf((float)(wy & 0xFFFFu), q_scale.y, q_lo.y); hi.y = __builtin_fmaf((float)(wy >> 16), q_scale.y, q_lo.y);
  lo.z = __builtin_fmaf((float)(wz & 0xFFFFu), q_scale.z, q_lo.z); hi.z = __builtin_fmaf((float)(wz >> 16), q_scale.z, q_lo.z);
}

// the dequantisation of the TLAS
__device__ __forceinline__ void tlas_dequant(const SceneDev& sc, F3& q_lo, F3& q_scale) {
  q_lo = mk3(sc.tlas_q_lo[0], sc.tlas_q_lo[1], sc.tlas_q_lo[2]); q_scale = mk3(sc.tlas_q_scale[0], sc.tlas_q_scale[1], sc.tlas_q_scale[2]);
}

// mag and the largest magnitude of the TLAS bounds, whichever is larger
__device__ __forceinline__ float tlas_magnitude(const SceneDev& sc, float mag) {
  for (int k = 0; k < 3; k++)
    mag = fmaxf(mag, fmaxf(__builtin_fabsf(sc.tlas_q_lo[k]), __builtin_fabsf(__builtin_fmaf(65535.0f, sc.tlas_q_scale[k], sc.tlas_q_lo[k]))));
  return mag;
}

// the counting forms: the wave's node visits and triangle tests into the query's counter block
__device__ __forceinline__ void walk_flush_counters(uint32_t* counters, unsigned long long cnt_nodes, unsigned long long cnt_tris) {
  for (int off = 32; off > 0; off >>= 1) {
    cnt_nodes += __shfl_down((unsigned long long)cnt_nodes, off);
    cnt_tris += __shfl_down((unsigned long long)cnt_tris, off);
  }
  if ((threadIdx.x & 63u) == 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(counters + CNT_NODE_VISITS), (unsigned long long)cnt_nodes);
    atomicAdd(reinterpret_cast<unsigned long long*>(counters + CNT_TRI_TESTS), (unsigned long long)cnt_tris);
  }
}

// The launch of a walk over the a.n records of `a`: k_query_init zeroes the chunk cursor (cnt_work(0, 0)), then the counting or the plain
// kernel on the persistent grid the spill area is sized for, no larger than the records need.
template <class Args>
void launch_walk(void (*plain)(Args), void (*counted)(Args), Args a, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s) {
  hipLaunchKernelGGL(k_query_init, dim3(1), dim3(64), 0, s, counters, a.n);
  a.cursor = counters + cnt_work(0, 0);
  const uint32_t blocks = min((uint32_t)cfg.trace_blocks, (a.n + 255u) / 256u);
  hipLaunchKernelGGL(counting ? counted : plain, dim3(blocks), dim3(256), 0, s, a);
}
