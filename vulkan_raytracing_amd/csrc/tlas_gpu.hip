// tlas_gpu.hip — the TLAS of one frame slot built (or refitted) on the GPU from device-resident instance records: what the
// driver does behind vkCmdBuildAccelerationStructuresKHR for the reference's TLAS (src/main.cpp:538-793, rebuilt every frame
// :2836-2861).  rt_set_instances builds the same TLAS on the host (binned SAH); rt_set_instances_device calls this file.
//
// One build, all on the context's build stream, one readback at the end:
//   k_tlas_init      the summary (error flags, bounds accumulators)
//   k_inst_records   one thread per instance: InstanceDev (w2o bit-identical to rt_api.cpp invert_affine), padded world box
//                    (the instance_world_box rule), scene and centroid bounds, mesh-index checks
//   LBVH             k_morton -> hipcub radix sort -> k_radix_tree (lbvh_kernels.h, shared with the BLAS builder)
//   k_tlas_refit     bottom-up boxes and subtree heights with one arrival flag per node; a refit (update) runs only this
//                    over the kept topology
//   k_tlas_quant     the dequantisation of quant_params (bvh_build.cpp) over the bounds, the depth
//   k_tlas_emit      32-byte BvhNodeQ nodes into the slot's TLAS region, interior links rebased to it, leaves ~instance
//   k_tlas_far       the object-space half of far_possible (rt_api.cpp) at the corners of G, OR-reduced
// Scratch grows with the instance count and is never freed between calls; nothing here allocates or synchronises per level.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstddef>
#include <string>

#include "lbvh_kernels.h"
#include "tlas_gpu.h"

namespace rt {
namespace {

// rt_instance (include/rt_api.h) as the kernels read it
struct RecDev {
  float transform[12];
  uint32_t custom_index_and_mask, sbt_offset_and_flags;
  uint64_t mesh;
};
static_assert(sizeof(RecDev) == 64, "RecDev mirrors rt_instance");

constexpr float BOX_NONE = 3.0e38f;   // instance_world_box of an empty mesh: lo = hi = 3e38 (no ray enters it)

__global__ void k_tlas_init(TlasSummary* s) {
  const int t = threadIdx.x;
  if (t == 0) { s->bad_mesh = 0xFFFFFFFFu; s->unbuilt = 0xFFFFFFFFu; s->far = 0u; s->depth = 0; s->blas_levels = 0; }
  if (t < 6) {
    s->bounds[t] = t < 3 ? 0xFFFFFFFFu : 0u;
    s->cbounds[t] = t < 3 ? 0xFFFFFFFFu : 0u;
  }
}

__global__ __launch_bounds__(256) void k_inst_records(const RecDev* rec, int n, const TlasMeshDev* meshes, int n_meshes, const uint32_t* types, int n_types,
                                                      InstanceDev* out, Box* boxes, TlasSummary* s) {
  __shared__ uint32_t s_b[12];
  __shared__ int s_levels;
  if (threadIdx.x < 12) s_b[threadIdx.x] = (threadIdx.x % 6) < 3 ? 0xFFFFFFFFu : 0u;
  if (threadIdx.x == 0) s_levels = 0;
  __syncthreads();
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const RecDev r = rec[i];
    InstanceDev d{};
    Box w;
    for (int k = 0; k < 3; k++) { w.lo[k] = BOX_NONE; w.hi[k] = BOX_NONE; }
    if (r.mesh >= (uint64_t)n_meshes) atomicMin(&s->bad_mesh, (uint32_t)i);
    else {
      const TlasMeshDev& m = meshes[r.mesh];
      if (!m.built) atomicMin(&s->unbuilt, (uint32_t)i);
      for (int k = 0; k < 12; k++) d.o2w[k] = r.transform[k];
      {
        // invert_affine (rt_api.cpp): binary64, the same operations in the same order (no contraction), rounded once
        const float* mm = r.transform;
        const double a = mm[0], b = mm[1], c = mm[2], dd = mm[4], e = mm[5], f = mm[6], g = mm[8], h = mm[9], ii = mm[10];
        const double tx = mm[3], ty = mm[7], tz = mm[11];
        const double c00 = e * ii - f * h, c01 = c * h - b * ii, c02 = b * f - c * e;
        const double c10 = f * g - dd * ii, c11 = a * ii - c * g, c12 = c * dd - a * f;
        const double c20 = dd * h - e * g, c21 = b * g - a * h, c22 = a * e - b * dd;
        const double det = a * c00 + b * c10 + c * c20;
        const double rr = 1.0 / det;
        const double q[9] = {c00 * rr, c01 * rr, c02 * rr, c10 * rr, c11 * rr, c12 * rr, c20 * rr, c21 * rr, c22 * rr};
        d.w2o[0] = (float)q[0]; d.w2o[1] = (float)q[1]; d.w2o[2] = (float)q[2];
        d.w2o[4] = (float)q[3]; d.w2o[5] = (float)q[4]; d.w2o[6] = (float)q[5];
        d.w2o[8] = (float)q[6]; d.w2o[9] = (float)q[7]; d.w2o[10] = (float)q[8];
        d.w2o[3] = (float)(-(q[0] * tx + q[1] * ty + q[2] * tz));
        d.w2o[7] = (float)(-(q[3] * tx + q[4] * ty + q[5] * tz));
        d.w2o[11] = (float)(-(q[6] * tx + q[7] * ty + q[8] * tz));
      }
      d.blas_root = m.blas_root;
      d.blas_root4 = m.blas_root4;
      d.mask = m.prim_count ? instance_mask_word(r.custom_index_and_mask, r.sbt_offset_and_flags) : 0u;   // an empty mesh is never entered
      for (int k = 0; k < 3; k++) { d.q_lo[k] = m.q_lo[k]; d.q_scale[k] = m.q_scale[k]; }
      d.custom_index = (int32_t)(r.custom_index_and_mask & 0xFFFFFFu);
      d.first_float = m.first_float;
      d.first_index = m.first_index;
      d.type = i < n_types ? types[i] : TYPE_BY_OBJECT_INDEX;
      d.cover_first = m.cover_first; d.cover_count = m.prim_count ? m.cover_count : 0u; d.prim_count = m.prim_count;
      // instance_world_box (rt_api.cpp): 8 transformed corners of the mesh bounds, padded against the binary32 roundings
      if (!(m.lo[0] > m.hi[0])) {
        for (int k = 0; k < 3; k++) { w.lo[k] = 3.0e38f; w.hi[k] = -3.0e38f; }
        float mag = 0.f;
        for (int cx = 0; cx < 8; cx++) {
          const double p[3] = {(cx & 1) ? m.hi[0] : m.lo[0], (cx & 2) ? m.hi[1] : m.lo[1], (cx & 4) ? m.hi[2] : m.lo[2]};
          for (int k = 0; k < 3; k++) {
            const double v = (double)r.transform[4 * k] * p[0] + (double)r.transform[4 * k + 1] * p[1] + (double)r.transform[4 * k + 2] * p[2] + (double)r.transform[4 * k + 3];
            w.lo[k] = fminf(w.lo[k], (float)v); w.hi[k] = fmaxf(w.hi[k], (float)v);
            mag = fmaxf(mag, (float)fabs(v));
          }
        }
        const float pad = 1e-5f * mag + 1e-30f;
        for (int k = 0; k < 3; k++) { w.lo[k] -= pad; w.hi[k] += pad; }
      }
      // instance_record_state (rt_api.cpp), the same two tests: a VOID record (an entry of the transform that is not finite, or a
      // padded box reaching INST_BOX_LIMIT) is the record of an empty mesh — mask word 0, BOX_NONE, nothing of it enters the bounds;
      // a record whose w2o is not finite keeps its world-space mask only, so no ray is ever transformed by that w2o
      bool fin = true, inv = true, inside = true;
      for (int k = 0; k < 12; k++) { fin = fin && __builtin_fabsf(r.transform[k]) <= 3.4028234e38f; inv = inv && __builtin_fabsf(d.w2o[k]) <= 3.4028234e38f; }
      for (int k = 0; k < 3; k++) inside = inside && __builtin_fabsf(w.lo[k]) < INST_BOX_LIMIT && __builtin_fabsf(w.hi[k]) < INST_BOX_LIMIT;
      if (!fin || !inside) {   // (an empty mesh arrives here as it is: mask 0, BOX_NONE)
        d.mask = 0u;
        for (int k = 0; k < 3; k++) { w.lo[k] = BOX_NONE; w.hi[k] = BOX_NONE; }
      } else if (!inv) d.mask &= ~0xFFu;
      if (m.built) atomicMax(&s_levels, m.levels);
    }
    out[i] = d;
    boxes[i] = w;
    if (w.lo[0] < INST_BOX_LIMIT)   // (boxes of empty meshes and of void records stay out of the bounds, as bvh2_bounds leaves them out)
      for (int k = 0; k < 3; k++) {
        atomicMin(&s_b[k], f2ord(w.lo[k])); atomicMax(&s_b[3 + k], f2ord(w.hi[k]));
        const float cen = 0.5f * w.lo[k] + 0.5f * w.hi[k];
        atomicMin(&s_b[6 + k], f2ord(cen)); atomicMax(&s_b[9 + k], f2ord(cen));
      }
  }
  __syncthreads();
  if (threadIdx.x < 3) { atomicMin(&s->bounds[threadIdx.x], s_b[threadIdx.x]); atomicMin(&s->cbounds[threadIdx.x], s_b[6 + threadIdx.x]); }
  else if (threadIdx.x < 6) { atomicMax(&s->bounds[threadIdx.x], s_b[threadIdx.x]); atomicMax(&s->cbounds[threadIdx.x], s_b[6 + threadIdx.x]); }
  else if (threadIdx.x == 6 && s_levels > 0) atomicMax(&s->blas_levels, s_levels);
}

// Bottom-up boxes over the radix tree (a build) or the kept topology (a refit, Vulkan UPDATE mode): every leaf climbs, the second
// arrival at a node owns the finished subtree below it, stores its box and height and climbs on.  flags must be zero.
__global__ __launch_bounds__(256) void k_tlas_refit(const Box* inst_boxes, const uint32_t* sorted_ids, int n, const int2* children, const int* parent_internal,
                                                    const int* parent_leaf, Box* node_boxes, int* height, uint32_t* flags) {
  const int leaf = blockIdx.x * blockDim.x + threadIdx.x;
  if (leaf >= n) return;
  int node = parent_leaf[leaf];
  while (node >= 0) {
    __threadfence();
    if (atomicAdd(&flags[node], 1u) == 0u) return;   // first arrival: the sibling subtree is not finished yet
    __threadfence();
    // (the acquire fence above invalidated this CU's L1, so plain loads see the sibling subtree's boxes)
    const int2 ch = children[node];
    const Box a = ch.x >= 0 ? node_boxes[ch.x] : inst_boxes[sorted_ids[~ch.x]];
    const Box b = ch.y >= 0 ? node_boxes[ch.y] : inst_boxes[sorted_ids[~ch.y]];
    const int ha = ch.x >= 0 ? height[ch.x] : 0, hb = ch.y >= 0 ? height[ch.y] : 0;
    node_boxes[node] = box_union(a, b);
    height[node] = 1 + max(ha, hb);
    node = parent_internal[node];
  }
}

// The radix tree is as deep as the keys make it: a level per bit in which neighbours differ, and further levels among equal keys.  The
// kernels' contract is a TLAS of at most TLAS_MAX_DEPTH interior levels (rt_device.h; the host builder enforces it), so a deeper radix
// tree is replaced by the BALANCED tree over the same Morton order: every range of leaves is split at its middle, ceil(log2 n) levels,
// 20 at the 2^20 instances the call accepts.  Numbering as in k_radix_tree (the left child of a split at m is node m, the right child
// node m + 1, the root node 0), so everything downstream is unchanged.  One thread per internal node finds its range from the root.
constexpr int TLAS_MAX_DEPTH = 20;
__global__ __launch_bounds__(256) void k_balanced_tree(int n, int2* children, int2* ranges, int* parent_internal, int* parent_leaf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n - 1) return;
  int l = 0, r = n - 1, self = 0;
  for (int step = 0; step < 32 && self != i; step++) {   // (node i lies below [l, r]: among l + 1 .. m on the left, m + 1 .. r - 1 on the right)
    const int m = l + ((r - l) >> 1);
    if (i <= m) { r = m; self = m; } else { l = m + 1; self = m + 1; }
  }
  if (self != i || r <= l) return;   // (cannot happen)
  const int m = l + ((r - l) >> 1);
  const int left = m > l ? m : ~l;
  const int right = m + 1 < r ? m + 1 : ~r;
  children[i] = make_int2(left, right);
  ranges[i] = make_int2(l, r);
  if (left >= 0) parent_internal[left] = i; else parent_leaf[~left] = i;
  if (right >= 0) parent_internal[right] = i; else parent_leaf[~right] = i;
  if (i == 0) parent_internal[0] = -1;
}

// quant_params (bvh_build.cpp) over the instance bounds, in binary64 like the host
__global__ void k_tlas_quant(TlasSummary* s, const int* height, int n) {
  const int k = threadIdx.x;
  if (k == 0) s->depth = n >= 2 ? height[0] : 0;
  if (k >= 3) return;
  double lo = 0.0, hi = 0.0;
  if (s->bounds[k] != 0xFFFFFFFFu) { lo = ord2f(s->bounds[k]); hi = ord2f(s->bounds[3 + k]); }
  if (lo > hi) { lo = hi = 0.0; }
  const double ext = hi - lo;
  const double scale = ext > 0 ? ext * (1.0 + 1e-6) / 65530.0 : 1e-30;
  s->q_lo[k] = (float)(lo - 2.0 * scale);
  s->q_scale[k] = (float)scale;
}

// quantize_bvh2_in (bvh_build.cpp): the doubles are re-derived from the float dequantisation, planes one quantum outside
__device__ __forceinline__ uint32_t q_clamp(double q) { const double t = (0.0 < q) ? q : 0.0; return (uint32_t)((t < 65535.0) ? t : 65535.0); }
__device__ __forceinline__ uint32_t q_axis(float lo, float hi, double base, double scale) {
  return q_clamp(floor(((double)lo - base) / scale) - 1.0) | (q_clamp(ceil(((double)hi - base) / scale) + 1.0) << 16);
}

// internal node i of the radix tree -> BvhNodeQ i of the slot's region; n == 1: the synthetic single-child root of quantize_bvh2
__global__ __launch_bounds__(256) void k_tlas_emit(const Box* inst_boxes, const uint32_t* sorted_ids, int n, const int2* children, const Box* node_boxes,
                                                   const TlasSummary* s, BvhNodeQ* out, int32_t node_base) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (n >= 2 ? n - 1 : 1)) return;
  double base[3], scale[3];
  for (int k = 0; k < 3; k++) { base[k] = s->q_lo[k]; scale[k] = s->q_scale[k]; }
  BvhNodeQ q{};
  if (n == 1) {
    const Box b = inst_boxes[0];
    for (int k = 0; k < 3; k++) { q.w[k] = q_axis(b.lo[k], b.hi[k], base[k], scale[k]); q.w[3 + k] = 0x0000FFFFu; }   // (absent child: inverted box)
    q.child0 = q.child1 = ~0;
  } else {
    const int2 ch = children[i];
    const int c[2] = {ch.x, ch.y};
    int32_t ref[2];
    for (int j = 0; j < 2; j++) {
      Box b;
      if (c[j] >= 0) { b = node_boxes[c[j]]; ref[j] = node_base + c[j]; }
      else { const uint32_t inst = sorted_ids[~c[j]]; b = inst_boxes[inst]; ref[j] = ~(int32_t)inst; }
      for (int k = 0; k < 3; k++) q.w[3 * j + k] = q_axis(b.lo[k], b.hi[k], base[k], scale[k]);
    }
    q.child0 = ref[0]; q.child1 = ref[1];
  }
  out[i] = q;
}

// far_possible's object-space test (rt_api.cpp) for every instance at the 8 corners of G: the TLAS's quantised bounds grown by their
// own extent on every side.  The test is one slab per axis, so passing at G's corners means passing everywhere inside G.
__global__ __launch_bounds__(256) void k_tlas_far(const RecDev* rec, int n, const TlasMeshDev* meshes, int n_meshes, const InstanceDev* inst, TlasSummary* s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  int far = 0;
  if (i < n && rec[i].mesh < (uint64_t)n_meshes && meshes[rec[i].mesh].prim_count && (inst[i].mask & 0xFFu) != 0u) {   // (no ray enters the others)
    const TlasMeshDev& m = meshes[rec[i].mesh];
    const double K = 0.99 * 2097152.0;
    double lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
      const double tlo = s->q_lo[k], thi = (double)s->q_lo[k] + 65535.0 * (double)s->q_scale[k];
      lo[k] = tlo - (thi - tlo); hi[k] = thi + (thi - tlo);
    }
    const float* w2o = inst[i].w2o;
    const double smin = fmin(fmin((double)m.q_scale[0], (double)m.q_scale[1]), (double)m.q_scale[2]);
    for (int cx = 0; cx < 8; cx++) {
      const double p[3] = {(cx & 1) ? hi[0] : lo[0], (cx & 2) ? hi[1] : lo[1], (cx & 4) ? hi[2] : lo[2]};
      for (int r = 0; r < 3; r++) {
        const double v = w2o[4 * r] * p[0] + w2o[4 * r + 1] * p[1] + w2o[4 * r + 2] * p[2] + w2o[4 * r + 3];
        if (!(fabs(m.q_lo[r] - v) <= K * smin)) far = 1;
      }
    }
  }
  if (__syncthreads_or(far) && threadIdx.x == 0) atomicOr(&s->far, 1u);
}

}  // namespace

void tlas_gpu_free(TlasGpu& g) {
  void* ps[] = {g.d_rec, g.d_boxes, g.d_keys, g.d_keys2, g.d_vals, g.d_vals2, g.d_sort_tmp, g.d_children, g.d_ranges, g.d_parent_int, g.d_parent_leaf,
                g.d_height, g.d_node_boxes, g.d_flags, g.d_types, g.d_sum};
  for (void* p : ps) if (p) hipFree(p);
  if (g.h_sum) hipHostFree(g.h_sum);
  if (g.ev_in) hipEventDestroy(g.ev_in);
  if (g.stream) hipStreamDestroy(g.stream);
  g = TlasGpu{};
}

int tlas_gpu_build(TlasGpu& g, const TlasBuildArgs& a, std::string& err) {
#define TG_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { err = std::string("HIP runtime exception: return code ") + std::to_string((int)e_) + " (" + hipGetErrorString(e_) + ") in " #expr; return 1; } } while (0)
  const int n = a.n;
  if (!g.stream) TG_TRY(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
  if (!g.ev_in) TG_TRY(hipEventCreateWithFlags(&g.ev_in, hipEventDisableTiming));
  if (!g.d_sum) TG_TRY(hipMalloc((void**)&g.d_sum, sizeof(TlasSummary)));
  if (!g.h_sum) TG_TRY(hipHostMalloc((void**)&g.h_sum, sizeof(TlasSummary), hipHostMallocDefault));
  if ((size_t)n > g.cap) {
    // grow-only: every array at the new capacity (the old topology goes with it: a refit needs the same n, which never grows)
    void** ps[] = {&g.d_rec, (void**)&g.d_boxes, (void**)&g.d_keys, (void**)&g.d_keys2, (void**)&g.d_vals, (void**)&g.d_vals2, &g.d_sort_tmp, (void**)&g.d_children,
                   (void**)&g.d_ranges, (void**)&g.d_parent_int, (void**)&g.d_parent_leaf, (void**)&g.d_height, (void**)&g.d_node_boxes, (void**)&g.d_flags};
    for (void** p : ps) { if (*p) TG_TRY(hipFree(*p)); *p = nullptr; }
    g.cap = 0; g.topo_n = 0; g.sort_bytes = 0;
    const size_t cap = ((size_t)n + 1023) & ~(size_t)1023;
    TG_TRY(hipMalloc(&g.d_rec, cap * sizeof(RecDev)));
    TG_TRY(hipMalloc((void**)&g.d_boxes, cap * sizeof(Box)));
    TG_TRY(hipMalloc((void**)&g.d_node_boxes, cap * sizeof(Box)));
    for (uint32_t** p : {&g.d_keys, &g.d_keys2, &g.d_vals, &g.d_vals2, &g.d_flags}) TG_TRY(hipMalloc((void**)p, cap * sizeof(uint32_t)));
    for (int** p : {&g.d_parent_int, &g.d_parent_leaf, &g.d_height}) TG_TRY(hipMalloc((void**)p, cap * sizeof(int)));
    TG_TRY(hipMalloc((void**)&g.d_children, cap * sizeof(int2)));
    TG_TRY(hipMalloc((void**)&g.d_ranges, cap * sizeof(int2)));
    TG_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, g.sort_bytes, g.d_keys, g.d_keys2, g.d_vals, g.d_vals2, (int)cap, 0, 30, g.stream));
    TG_TRY(hipMalloc(&g.d_sort_tmp, g.sort_bytes));
    g.cap = cap;
  }
  if (a.refit && g.topo_n != n) { err = "TLAS refit without a device topology of the same instance count"; return 1; }
  hipStream_t s = g.stream;
  if (a.d_src != g.d_rec) {
    // the caller's records, read in the caller's stream order; from here on the caller may overwrite its buffer
    TG_TRY(hipMemcpyAsync(g.d_rec, a.d_src, (size_t)n * sizeof(RecDev), hipMemcpyDeviceToDevice, a.src_stream));
    TG_TRY(hipEventRecord(g.ev_in, a.src_stream));
    TG_TRY(hipStreamWaitEvent(s, g.ev_in, 0));
  }
  if (a.n_types > 0) {
    if ((size_t)a.n_types > g.types_cap) {
      if (g.d_types) TG_TRY(hipFree(g.d_types));
      g.d_types = nullptr; g.types_cap = 0;
      TG_TRY(hipMalloc((void**)&g.d_types, (size_t)a.n_types * sizeof(uint32_t)));
      g.types_cap = (size_t)a.n_types;
    }
    TG_TRY(hipMemcpyAsync(g.d_types, a.h_types, (size_t)a.n_types * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  }
  const RecDev* rec = (const RecDev*)g.d_rec;
  Box* boxes = (Box*)g.d_boxes;
  Box* node_boxes = (Box*)g.d_node_boxes;
  const unsigned nb = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_tlas_init, dim3(1), dim3(64), 0, s, g.d_sum);
  hipLaunchKernelGGL(k_inst_records, dim3(nb), dim3(256), 0, s, rec, n, a.meshes, a.n_meshes, g.d_types, a.n_types, a.d_inst, boxes, g.d_sum);
  if (n >= 2) {
    if (!a.refit) {
      hipLaunchKernelGGL(k_morton, dim3(nb), dim3(256), 0, s, boxes, (uint32_t)n, (const uint32_t*)((const char*)g.d_sum + offsetof(TlasSummary, cbounds)), g.d_keys, g.d_vals);
      size_t bytes = g.sort_bytes;
      TG_TRY(hipcub::DeviceRadixSort::SortPairs(g.d_sort_tmp, bytes, g.d_keys, g.d_keys2, g.d_vals, g.d_vals2, n, 0, 30, s));
      hipLaunchKernelGGL(k_radix_tree, dim3(nb), dim3(256), 0, s, g.d_keys2, n, g.d_children, g.d_ranges, g.d_parent_int, g.d_parent_leaf);
    }
  }
  // boxes bottom-up over the topology, the dequantisation and the depth, the nodes, the far flag, one readback; once more over the
  // balanced tree when the radix tree turns out deeper than the contract allows
  const int n_nodes = n >= 2 ? n - 1 : 1;
  for (int pass = 0; pass < 2; pass++) {
    if (pass == 1) {
      if (a.refit || n < 2 || g.h_sum->depth <= TLAS_MAX_DEPTH) break;
      hipLaunchKernelGGL(k_balanced_tree, dim3(nb), dim3(256), 0, s, n, g.d_children, g.d_ranges, g.d_parent_int, g.d_parent_leaf);   // (the radix tree is too deep)
    }
    if (n >= 2) {
      TG_TRY(hipMemsetAsync(g.d_flags, 0, (size_t)(n - 1) * sizeof(uint32_t), s));
      hipLaunchKernelGGL(k_tlas_refit, dim3(nb), dim3(256), 0, s, boxes, g.d_vals2, n, g.d_children, g.d_parent_int, g.d_parent_leaf, node_boxes, g.d_height, g.d_flags);
    }
    hipLaunchKernelGGL(k_tlas_quant, dim3(1), dim3(64), 0, s, g.d_sum, g.d_height, n);
    hipLaunchKernelGGL(k_tlas_emit, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, s, boxes, g.d_vals2, n, g.d_children, node_boxes, g.d_sum, a.d_nodes, a.node_base);
    hipLaunchKernelGGL(k_tlas_far, dim3(nb), dim3(256), 0, s, rec, n, a.meshes, a.n_meshes, a.d_inst, g.d_sum);
    TG_TRY(hipGetLastError());
    TG_TRY(hipMemcpyAsync(g.h_sum, g.d_sum, sizeof(TlasSummary), hipMemcpyDeviceToHost, s));
    TG_TRY(hipStreamSynchronize(s));
  }
  if (!a.refit) g.topo_n = n;
  return 0;
#undef TG_TRY
}

}  // namespace rt
