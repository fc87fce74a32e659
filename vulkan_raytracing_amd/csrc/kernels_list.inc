// kernels_list.inc — included by kernels.hip after kernels_refs.inc (product and alt translation units alike).
// rt_overlap_*_device_list: the whole candidate set of every record in CSR form (DESIGN.md §5 "Overlap lists").  Three steps in stream order:
//
//  * count: the count-only walk of the capped call (k == 0), unchanged, into n counts of the query workspace;
//  * scan: k_list_scan_sums, k_list_scan_tops, k_list_scan_offsets turn the uint32 counts into n + 1 uint64 row starts, the last of
//    them the total.  Every sum is a uint64: n counts below 2^32 each do not fit anything less;
//  * fill: the LIST instantiations of overlap_body (walk_overlap.inc: k_list_boxes, k_list_triangles, k_list_refs) walk again and write
//    every candidate into its row.  A lane passes over a record whose row is empty or ends beyond the capacity.  A row of at most
//    RT_LIST_INSERT_MAX entries is kept sorted by insertion, as the capped kernels keep theirs; a longer one is written in walk order
//    and its record goes onto a worklist.  k_list_sort, one workgroup per listed row, sorts such a row in place by (inst, prim).
//
// The sort is a bitonic network whose comparators all put the smaller key at the lower index (the first step of a merge compares
// mirrored positions).  Positions at and beyond the row's length then behave as keys above all others that never move, so a row of any
// length is sorted without padding: a comparator with a partner beyond the row is passed over.  A row of at most RT_LIST_LDS_TILE
// entries is sorted in LDS; a longer one tile by tile in LDS, the steps whose distance reaches across tiles on the row in global memory
// (the workgroup's own writes, read back behind a barrier).  Keys are unique within a row, so the sorted row is unique whatever order
// the walk wrote.  The network is list_sort_body, a template over what a row's records and keys are: k_list_sort instantiates it for
// (inst, prim) rows, k_ipairs_sort (kernels_ipairs.inc) for the `against` words of rt_inst_ref rows.

// ---- scan
constexpr uint32_t LIST_SCAN_ITEMS = 8u, LIST_SCAN_TILE = 256u * LIST_SCAN_ITEMS;   // counts per thread and per workgroup

// the inclusive sum of v over the workgroup's 256 threads in thread order; total: the whole sum.  s_wave: 4 words of LDS.
__device__ __forceinline__ unsigned long long list_block_scan(unsigned long long v, unsigned long long* s_wave, unsigned long long& total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long o = __shfl_up(v, off);
    if (lane >= (uint32_t)off) v += o;
  }
  __syncthreads();   // (the previous use of s_wave is over)
  if (lane == 63u) s_wave[wave] = v;
  __syncthreads();
  unsigned long long before = 0;
  for (uint32_t w = 0; w < 4u; w++) { const unsigned long long t = s_wave[w]; if (w < wave) before += t; }
  total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  return v + before;
}

// the sum of the counts of scan tile b (counts at and beyond n are zero)
__global__ __launch_bounds__(256) void k_list_scan_sums(const uint32_t* __restrict__ counts, uint32_t n, unsigned long long* __restrict__ sums) {
  __shared__ unsigned long long s_wave[4];
  const unsigned long long base = (unsigned long long)blockIdx.x * LIST_SCAN_TILE + (unsigned long long)threadIdx.x * LIST_SCAN_ITEMS;
  unsigned long long v = 0;
  for (uint32_t e = 0; e < LIST_SCAN_ITEMS; e++) if (base + e < n) v += counts[base + e];
  unsigned long long total;
  list_block_scan(v, s_wave, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// the tile sums into their exclusive prefix, in place: one workgroup, 256 sums a trip
__global__ __launch_bounds__(256) void k_list_scan_tops(unsigned long long* sums, uint32_t n_tiles) {
  __shared__ unsigned long long s_wave[4];
  unsigned long long running = 0;
  for (uint32_t base = 0; base < n_tiles; base += 256u) {
    const uint32_t i = base + threadIdx.x;
    const unsigned long long v = i < n_tiles ? sums[i] : 0ull;
    unsigned long long total;
    const unsigned long long incl = list_block_scan(v, s_wave, total);
    if (i < n_tiles) sums[i] = running + incl - v;
    running += total;
  }
}

// offsets[i] = the sum of the counts before i, for every i <= n
__global__ __launch_bounds__(256) void k_list_scan_offsets(const uint32_t* __restrict__ counts, uint32_t n, const unsigned long long* __restrict__ sums,
                                                            unsigned long long* __restrict__ offsets) {
  __shared__ unsigned long long s_wave[4];
  const unsigned long long base = (unsigned long long)blockIdx.x * LIST_SCAN_TILE + (unsigned long long)threadIdx.x * LIST_SCAN_ITEMS;
  uint32_t c[LIST_SCAN_ITEMS];
  unsigned long long v = 0;
  for (uint32_t e = 0; e < LIST_SCAN_ITEMS; e++) { c[e] = base + e < n ? counts[base + e] : 0u; v += c[e]; }
  unsigned long long total;
  unsigned long long at = list_block_scan(v, s_wave, total) - v + sums[blockIdx.x];
  for (uint32_t e = 0; e < LIST_SCAN_ITEMS; e++) {
    if (base + e <= n) offsets[base + e] = at;
    at += c[e];
  }
}

// the n + 1 offsets of n counts; sums: ceil((n + 1) / LIST_SCAN_TILE) words of the workspace (list_scan_tiles)
uint32_t list_scan_tiles(uint32_t n) { return (uint32_t)(((uint64_t)n + 1u + LIST_SCAN_TILE - 1u) / LIST_SCAN_TILE); }
void launch_list_scan(const uint32_t* counts, uint32_t n, unsigned long long* sums, unsigned long long* offsets, hipStream_t s) {
  const uint32_t tiles = list_scan_tiles(n);
  hipLaunchKernelGGL(k_list_scan_sums, dim3(tiles), dim3(256), 0, s, counts, n, sums);
  hipLaunchKernelGGL(k_list_scan_tops, dim3(1), dim3(256), 0, s, sums, tiles);
  hipLaunchKernelGGL(k_list_scan_offsets, dim3(tiles), dim3(256), 0, s, counts, n, (const unsigned long long*)sums, offsets);
}

// ---- fill: the walks
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_list_boxes(OverlapArgs a) { overlap_body<OverlapBox, false, false, true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_list_boxes_count(OverlapArgs a) { overlap_body<OverlapBox, true, false, true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_list_triangles(OverlapArgs a) { overlap_body<OverlapTriangle, false, false, true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_list_triangles_count(OverlapArgs a) { overlap_body<OverlapTriangle, true, false, true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_list_refs(OverlapArgs a) { overlap_body<OverlapTriangle, false, true, true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_list_refs_count(OverlapArgs a) { overlap_body<OverlapTriangle, true, true, true>(a); }

// ---- sort
constexpr uint32_t LIST_TILE = RT_LIST_LDS_TILE;
static_assert(LIST_TILE >= 512u && (LIST_TILE & (LIST_TILE - 1u)) == 0u, "RT_LIST_LDS_TILE: a power of two, two entries per thread at the least");
static_assert(RT_LIST_INSERT_MAX >= 1 && (uint32_t)RT_LIST_INSERT_MAX < LIST_TILE, "RT_LIST_INSERT_MAX: below the tile");

// What k_list_sort permutes is a shape of its own (a sibling kernel sorts other rows with the same network: kernels_ipairs.inc):
//    Rec                       the records of a row
//    Key                       what orders them, unique within a row
//    static Key key(rows, i)   the key of record i
//    static void put(rows, i, key)   record i takes the key (and nothing else of it changes)
// The rows of the overlap lists: (inst, prim), both non-negative, as one key in (inst, prim) order
struct ListIds {
  typedef IdRec Rec;
  typedef unsigned long long Key;
  __device__ __forceinline__ static Key key(const IdRec* ids, size_t i) {
    const int32_t* w = reinterpret_cast<const int32_t*>(ids + i);   // (rows are 4-byte aligned)
    return ((unsigned long long)(uint32_t)w[0] << 32) | (unsigned long long)(uint32_t)w[1];
  }
  __device__ __forceinline__ static void put(IdRec* ids, size_t i, Key key) {
    int32_t* w = reinterpret_cast<int32_t*>(ids + i);
    w[0] = (int32_t)(uint32_t)(key >> 32); w[1] = (int32_t)(uint32_t)key;
  }
};
// pair p of a step: the lower index of the p-th pair whose members differ in the bit h (a power of two)
__device__ __forceinline__ uint32_t list_pair(uint32_t p, uint32_t h) { return ((p & ~(h - 1u)) << 1) | (p & (h - 1u)); }
// the smallest power of two that is no less than m (m >= 2)
__device__ __forceinline__ uint32_t list_pow2(uint32_t m) { return 1u << (32 - __builtin_clz(m - 1u)); }

// One step over the m keys of s (LDS): pairs (i, i ^ (k - 1)) of blocks of k when flip, (i, i | h) otherwise; then the barrier.
// pairs: half the power of two that holds m; a pair beyond it has no member below m.
template <class R>
__device__ __forceinline__ void list_lds_step(typename R::Key* s, uint32_t m, uint32_t pairs, uint32_t h, bool flip) {
  for (uint32_t p = threadIdx.x; p < pairs; p += 256u) {
    const uint32_t i = list_pair(p, h), q = flip ? (i ^ (2u * h - 1u)) : (i | h);
    if (q < m) {
      const typename R::Key x = s[i], y = s[q];
      if (x > y) { s[i] = y; s[q] = x; }
    }
  }
  __syncthreads();
}
// the same step over the len keys of a row in global memory (distances of a tile and more)
template <class R>
__device__ __forceinline__ void list_global_step(typename R::Rec* row, uint32_t len, uint32_t pairs, uint32_t h, bool flip) {
  for (uint32_t p = threadIdx.x; p < pairs; p += 256u) {
    const uint32_t i = list_pair(p, h), q = flip ? (i ^ (2u * h - 1u)) : (i | h);
    if (q < len) {
      const typename R::Key x = R::key(row, i), y = R::key(row, q);
      if (x > y) { R::put(row, i, y); R::put(row, q, x); }
    }
  }
  __syncthreads();
}
template <class R>
__device__ __forceinline__ void list_tile_load(typename R::Key* s, const typename R::Rec* row, uint32_t m) {
  for (uint32_t i = threadIdx.x; i < m; i += 256u) s[i] = R::key(row, i);
  __syncthreads();
}
template <class R>
__device__ __forceinline__ void list_tile_store(const typename R::Key* s, typename R::Rec* row, uint32_t m) {
  for (uint32_t i = threadIdx.x; i < m; i += 256u) R::put(row, i, s[i]);
  __syncthreads();   // (the next load of this LDS, the next reader of the row)
}

// the sort of every listed row, one workgroup per row; s_keys: LIST_TILE keys of LDS
template <class R>
__device__ __forceinline__ void list_sort_body(typename R::Rec* rows, const unsigned long long* offsets, const uint32_t* worklist, const uint32_t* work_count,
                                               typename R::Key* s_keys) {
  const uint32_t n_work = *work_count;
  for (uint32_t w = blockIdx.x; w < n_work; w += gridDim.x) {
    const uint32_t rec = worklist[w];
    const unsigned long long o0 = offsets[rec];
    const uint32_t len = (uint32_t)(offsets[rec + 1u] - o0);
    if (len < 2u) continue;
    typename R::Rec* row = rows + o0;
    // every tile sorted by itself (a row that fits: the whole sort)
    for (uint32_t b = 0; b < len; b += LIST_TILE) {
      const uint32_t m = min(LIST_TILE, len - b);
      list_tile_load<R>(s_keys, row + b, m);
      if (m >= 2u) {
        const uint32_t P = list_pow2(m);
        for (uint32_t k = 2u; k <= P; k <<= 1) {
          list_lds_step<R>(s_keys, m, P >> 1, k >> 1, true);
          for (uint32_t h = k >> 2; h > 0u; h >>= 1) list_lds_step<R>(s_keys, m, P >> 1, h, false);
        }
      }
      list_tile_store<R>(s_keys, row + b, m);
    }
    if (len <= LIST_TILE) continue;
    // merges of two, four, ... tiles: the steps that reach across tiles on the row itself, the rest tile by tile in LDS
    const uint32_t P = list_pow2(len);
    for (uint32_t k = 2u * LIST_TILE; k <= P; k <<= 1) {
      list_global_step<R>(row, len, P >> 1, k >> 1, true);
      for (uint32_t h = k >> 2; h >= LIST_TILE; h >>= 1) list_global_step<R>(row, len, P >> 1, h, false);
      for (uint32_t b = 0; b < len; b += LIST_TILE) {
        const uint32_t m = min(LIST_TILE, len - b);
        list_tile_load<R>(s_keys, row + b, m);
        for (uint32_t h = LIST_TILE >> 1; h > 0u; h >>= 1) list_lds_step<R>(s_keys, m, LIST_TILE >> 1, h, false);
        list_tile_store<R>(s_keys, row + b, m);
      }
    }
  }
}

struct ListSortArgs {
  IdRec* ids;
  const unsigned long long* offsets;
  const uint32_t* worklist;
  const uint32_t* work_count;
};

__global__ __launch_bounds__(256) void k_list_sort(ListSortArgs a) {
  __shared__ unsigned long long s_keys[LIST_TILE];
  list_sort_body<ListIds>(a.ids, a.offsets, a.worklist, a.work_count, s_keys);
}

// ---- launch.  work: 1 + n words (the number of listed rows, then the rows).
void launch_overlap_list(OverlapShape shape, const SceneDev& sc, const float4* records, uint32_t cull_mask, const float* inst_scale, const unsigned long long* offsets,
                         void* ids, uint64_t capacity, uint32_t* work, uint32_t n, int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg,
                         hipStream_t s) {
  static void (*const kernels[3][2])(OverlapArgs) = {{k_list_boxes, k_list_boxes_count}, {k_list_triangles, k_list_triangles_count}, {k_list_refs, k_list_refs_count}};
  OverlapArgs a = overlap_args(sc, records, cull_mask, inst_scale, ids, n, ovf_stack, counters);
  a.offsets = offsets; a.capacity = capacity; a.work_count = work; a.worklist = work + 1;   // (k = 0, any = 0, no counts)
  hipMemsetAsync(work, 0, sizeof(uint32_t), s);
  launch_walk(kernels[(int)shape][0], kernels[(int)shape][1], a, counters, counting, cfg, s);
  ListSortArgs t{(IdRec*)ids, offsets, work + 1, work};
  hipLaunchKernelGGL(k_list_sort, dim3(min((uint32_t)cfg.trace_blocks, n)), dim3(256), 0, s, t);
}
