// blas_refit.hip — one mesh's BLAS refitted on the GPU from new vertices (rt_refit_blas_device): Vulkan's BLAS update
// (VK_BUILD_ACCELERATION_STRUCTURE_MODE_UPDATE_KHR, src = dst) over a device vertex buffer.  The tree topology and the cache-line
// layout link_blas gave the mesh's nodes stay; everything derived from vertex positions is recomputed in place in the scene's
// linked arrays, on one stream, with one readback at the end:
//   (copy)           the caller's vertices into the scene's vertex buffer, in the caller's stream order
//   k_refit_parents  once per mesh and link: the parent of every node slot from the child links; filler slots are marked
//   k_refit_check    the non-finite-position flag over the vertex span
//   k_refit_leaves   one thread per node slot: the 48-byte packets of its leaf children (k_emit_tris' arithmetic) and their float
//                    boxes (k_tri_boxes' vertex boxes), then the climb: one arrival counter per node, the last arrival unites the
//                    two child boxes and goes on to the parent; the root's box goes to the summary
//   k_refit_quant    the dequantisation from the root box (blas_quant.h, the builders' rule) into the summary and the mesh table
//   k_refit_emit     both child boxes of every node re-quantised (two quanta of margin; an absent child gets the inverted box)
// A refit that met a non-finite position (or an inconsistent graph) writes no planes, frontier boxes or dequantisation: the mesh table
// marks the mesh not built, and the next good refit recomputes every packet and box.
//   k_refit_cover    the mesh's frontier boxes (k_cover) re-emitted from the new planes over the cut link_blas chose
// Nothing synchronises per tree level; the scratch (blas_refit.h) grows only.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>

#include "blas_quant.h"
#include "blas_refit.h"
#include "lbvh_kernels.h"

namespace rt {
namespace {

constexpr int32_t PARENT_ROOT = -1, PARENT_FILLER = -2;

// The absent child of a synthetic single-child root (quantize_bvh2) repeats its sibling's link; no two children of a tree share one.
// Presence is read from the links, which a refit never writes, and never from the planes, which it rewrites: a refit of bad
// vertices can leave any box empty, and an empty box quantises to the same inverted planes as the absent child.  Slot 1 is the
// absent one here; k_refit_emit gives it the inverted box ("never", 0x0000FFFF per axis) and slot 0 the child's box.
constexpr uint32_t PLANES_NEVER = 0x0000FFFFu;
__device__ __forceinline__ bool child_absent(const BvhNodeQ& q, int k) { return k == 1 && q.child1 == q.child0; }
__device__ __forceinline__ int children_of(const BvhNodeQ& q) { return q.child1 == q.child0 ? 1 : 2; }

__device__ __forceinline__ void box_store(float* p, const Box& b) { p[0] = b.lo[0]; p[1] = b.lo[1]; p[2] = b.lo[2]; p[3] = b.hi[0]; p[4] = b.hi[1]; p[5] = b.hi[2]; }
__device__ __forceinline__ Box box_load(const float* p) { Box b; b.lo[0] = p[0]; b.lo[1] = p[1]; b.lo[2] = p[2]; b.hi[0] = p[3]; b.hi[1] = p[4]; b.hi[2] = p[5]; return b; }
__device__ __forceinline__ Box box_none() { Box b; for (int k = 0; k < 3; k++) { b.lo[k] = 3.0e38f; b.hi[k] = -3.0e38f; } return b; }

// One arrival at a node (cdna_hip_programming.md §6 Guideline 16, per lane): the boxes this lane stored are released at agent scope
// before the counter moves; the lane that completes the count acquires before it reads the boxes the other arrivals stored.
__device__ __forceinline__ bool arrive(uint32_t* flag, uint32_t add, uint32_t need) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const uint32_t old = __hip_atomic_fetch_add(flag, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (old + add != need) return false;   // (exactly once per node: a corrupt graph cannot make a node climb twice)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return true;
}

// nodes / parent: the mesh's slots (local index i = global - node_base).  The treelet layout fills the slots it cannot use with
// copies of the mesh's root (link_blas treelet_layout): the same links as slot 0, which no other node of a tree has.
__global__ __launch_bounds__(256) void k_refit_parents(const BvhNodeQ* nodes, uint32_t count, int32_t node_base, int32_t* parent, RefitSummary* s) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const BvhNodeQ q = nodes[i];
  if (i != 0 && q.child0 == nodes[0].child0 && q.child1 == nodes[0].child1) { parent[i] = PARENT_FILLER; return; }
  const int32_t ch[2] = {q.child0, q.child1};
#pragma unroll
  for (int k = 0; k < 2; k++) {
    if (ch[k] < 0 || child_absent(q, k)) continue;
    const int64_t local = (int64_t)ch[k] - node_base;
    if (local <= 0 || local >= (int64_t)count) { atomicOr(&s->bad, 1u); continue; }
    parent[local] = (int32_t)((i << 1) | (uint32_t)k);
  }
}

__global__ __launch_bounds__(256) void k_refit_check(const float* verts6, uint32_t nv, RefitSummary* s) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (v < nv) {
    const float* p = verts6 + 6ull * v;
    bad = !(isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]));
  }
  if (__syncthreads_or(bad) && threadIdx.x == 0) atomicOr(&s->nonfinite, 1u);
}

// verts6 / idx: the mesh's first vertex float and first index (object-local indices).  cbox / flags: the mesh's slots.
__global__ __launch_bounds__(256) void k_refit_leaves(const BvhNodeQ* nodes, uint32_t count, const int32_t* parent, const float* verts6, uint32_t span_floats,
                                                      const uint32_t* idx, uint32_t prim_count, float4* tris, uint32_t tri_base, float* cbox, uint32_t* flags,
                                                      RefitSummary* s) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count || parent[i] == PARENT_FILLER) return;
  const BvhNodeQ q = nodes[i];
  const int32_t ch[2] = {q.child0, q.child1};
  uint32_t have = 0;
#pragma unroll
  for (int k = 0; k < 2; k++) {
    if (ch[k] >= 0 || child_absent(q, k)) continue;
    const uint32_t ref = (uint32_t)(~ch[k]), first = ref >> 3, cnt = (ref & 7u) + 1u;
    Box b = box_none();
    if (first < tri_base || first + cnt > tri_base + prim_count) atomicOr(&s->bad, 1u);
    else
      for (uint32_t j = first; j < first + cnt; j++) {
        const uint32_t p = __float_as_uint(tris[3ull * j + 2].y);   // (the prim id and the leaf order stay)
        if (p >= prim_count) { atomicOr(&s->bad, 1u); continue; }
        const uint32_t i0 = idx[3ull * p + 0], i1 = idx[3ull * p + 1], i2 = idx[3ull * p + 2];
        if (6ull * i0 + 6 > span_floats || 6ull * i1 + 6 > span_floats || 6ull * i2 + 6 > span_floats) { atomicOr(&s->bad, 1u); continue; }
        const float* v0 = verts6 + 6ull * i0;
        const float* v1 = verts6 + 6ull * i1;
        const float* v2 = verts6 + 6ull * i2;
        // k_emit_tris: e1 = v1 - v0, e2 = v2 - v0 rounded once in binary32
        const float e1x = v1[0] - v0[0], e1y = v1[1] - v0[1], e1z = v1[2] - v0[2];
        const float e2x = v2[0] - v0[0], e2y = v2[1] - v0[1], e2z = v2[2] - v0[2];
        tris[3ull * j + 0] = make_float4(v0[0], v0[1], v0[2], e1x);
        tris[3ull * j + 1] = make_float4(e1y, e1z, e2x, e2y);
        tris[3ull * j + 2] = make_float4(e2z, __uint_as_float(p), 0.f, 0.f);
        // k_tri_boxes: the box of the three vertices
#pragma unroll
        for (int a = 0; a < 3; a++) {
          b.lo[a] = fminf(b.lo[a], v0[a]); b.hi[a] = fmaxf(b.hi[a], v0[a]);
          b.lo[a] = fminf(b.lo[a], v1[a]); b.hi[a] = fmaxf(b.hi[a], v1[a]);
          b.lo[a] = fminf(b.lo[a], v2[a]); b.hi[a] = fmaxf(b.hi[a], v2[a]);
        }
      }
    box_store(cbox + 12ull * i + 6 * k, b);
    have++;
  }
  if (have == 0) return;
  // the climb: this slot is complete once every present child has arrived (its own leaves count at once)
  uint32_t node = i;
  uint32_t need = (uint32_t)children_of(q);
  if (have != need && !arrive(&flags[node], have, need)) return;
  for (uint32_t steps = 0; steps <= count; steps++) {
    const BvhNodeQ nq = nodes[node];
    Box u = box_none();
#pragma unroll
    for (int k = 0; k < 2; k++) {
      if (child_absent(nq, k)) continue;
      const Box c = box_load(cbox + 12ull * node + 6 * k);
#pragma unroll
      for (int a = 0; a < 3; a++) { u.lo[a] = fminf(u.lo[a], c.lo[a]); u.hi[a] = fmaxf(u.hi[a], c.hi[a]); }
    }
    const int32_t p = parent[node];
    if (p < 0) {
      if (p == PARENT_ROOT && node == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) { s->root_lo[a] = u.lo[a]; s->root_hi[a] = u.hi[a]; }
        s->root_done = 1u;
      } else atomicOr(&s->bad, 1u);   // (a slot no node links to)
      return;
    }
    const uint32_t up = (uint32_t)p >> 1;
    if (up >= count) { atomicOr(&s->bad, 1u); return; }
    box_store(cbox + 12ull * up + 6 * (p & 1), u);
    node = up;
    need = (uint32_t)children_of(nodes[node]);
    if (!arrive(&flags[node], 1u, need)) return;
  }
  atomicOr(&s->bad, 1u);
}

// ok(): the climb finished over finite vertices.  Otherwise the planes, the frontier boxes and the dequantisation of the mesh stay as
// they were and only `built` drops to 0: the mesh is unusable until a good refit, which recomputes every packet and box anyway.
__device__ __forceinline__ bool refit_ok(const RefitSummary* s) { return !(s->nonfinite | s->bad) && s->root_done; }

__global__ void k_refit_quant(RefitSummary* s, TlasMeshDev* entry) {
  const int k = threadIdx.x;
  if (k >= 3) return;
  if (k == 0) entry->built = refit_ok(s) ? 1u : 0u;   // (a mesh with a non-finite position is not built)
  if (!refit_ok(s)) return;
  const float lo = s->root_lo[k], hi = s->root_hi[k];
  float q_lo, q_scale;
  blas_quant_axis_params(lo, hi, &q_lo, &q_scale);
  s->q_lo[k] = q_lo; s->q_scale[k] = q_scale;
  entry->q_lo[k] = q_lo; entry->q_scale[k] = q_scale;
  entry->lo[k] = lo; entry->hi[k] = hi;
}

__global__ __launch_bounds__(256) void k_refit_emit(BvhNodeQ* nodes, uint32_t count, const int32_t* parent, const float* cbox, const RefitSummary* s) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count || parent[i] == PARENT_FILLER || !refit_ok(s)) return;
  BvhNodeQ q = nodes[i];
  float base[3], scale[3];
#pragma unroll
  for (int a = 0; a < 3; a++) { base[a] = s->q_lo[a]; scale[a] = s->q_scale[a]; }
#pragma unroll
  for (int k = 0; k < 2; k++) {
    if (child_absent(q, k)) { q.w[3 * k] = q.w[3 * k + 1] = q.w[3 * k + 2] = PLANES_NEVER; continue; }
    const Box b = box_load(cbox + 12ull * i + 6 * k);
#pragma unroll
    for (int a = 0; a < 3; a++) q.w[3 * k + a] = quant_box_axis(b.lo[a], b.hi[a], base[a], scale[a]);
  }
  nodes[i] = q;
}

// link_blas's emit(): a child box dequantised from its planes, padded by 1e-6 of its coordinates' magnitude
__global__ __launch_bounds__(256) void k_refit_cover(const BvhNodeQ* nodes, int32_t node_lo, int32_t node_hi, const uint32_t* src, uint32_t count, RefitSummary* s,
                                                     float* out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count || !refit_ok(s)) return;
  const uint32_t g = src[j] >> 1, k = src[j] & 1u;
  if ((int64_t)g < node_lo || (int64_t)g >= node_hi) { atomicOr(&s->bad, 1u); return; }
  const BvhNodeQ q = nodes[g];
  float lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const uint32_t w = q.w[3 * k + a];
    const uint32_t pl = w & 0xFFFFu, ph = w >> 16;
    lo[a] = s->q_lo[a] + (float)pl * s->q_scale[a]; hi[a] = s->q_lo[a] + (float)ph * s->q_scale[a];
    const float pad = 1e-6f * (fabsf(lo[a]) + fabsf(hi[a]));
    lo[a] -= pad; hi[a] += pad;
  }
  float* o = out + 6ull * j;
  o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = hi[0]; o[4] = hi[1]; o[5] = hi[2];
}

}  // namespace

int blas_refit_reserve(BlasRefitScratch& r, size_t n_slots, bool* grown, std::string& err) {
  *grown = false;
  if (n_slots <= r.parent_cap) return 0;
  if (r.d_parent) hipFree(r.d_parent);
  r.d_parent = nullptr; r.parent_cap = 0;
  const size_t cap = (n_slots + 1023) & ~(size_t)1023;
  hipError_t e = hipMalloc((void**)&r.d_parent, cap * sizeof(int32_t));
  if (e != hipSuccess) { err = std::string("HIP runtime exception: return code ") + std::to_string((int)e) + " (" + hipGetErrorString(e) + ") in hipMalloc(d_parent)"; return 1; }
  r.parent_cap = cap; *grown = true;
  return 0;
}

void blas_refit_free(BlasRefitScratch& r) {
  for (void* p : {(void*)r.d_parent, (void*)r.d_flags, (void*)r.d_cbox, (void*)r.d_sum}) if (p) hipFree(p);
  if (r.h_sum) hipHostFree(r.h_sum);
  for (hipEvent_t e : {r.ev_in, r.ev_t0, r.ev_t1}) if (e) hipEventDestroy(e);
  r = BlasRefitScratch{};
}

int blas_refit(BlasRefitScratch& r, const BlasRefitArgs& a, std::string& err) {
#define BR_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { err = std::string("HIP runtime exception: return code ") + std::to_string((int)e_) + " (" + hipGetErrorString(e_) + ") in " #expr; return 1; } } while (0)
  if (!a.node_count || (size_t)a.node_base + a.node_count > r.parent_cap) { err = "BLAS refit: the mesh's node range is not covered by the kept parents"; return 1; }
  if (!r.ev_in) BR_TRY(hipEventCreateWithFlags(&r.ev_in, hipEventDisableTiming));
  if (!r.d_sum) BR_TRY(hipMalloc((void**)&r.d_sum, sizeof(RefitSummary)));
  if (!r.h_sum) BR_TRY(hipHostMalloc((void**)&r.h_sum, sizeof(RefitSummary), hipHostMallocDefault));
  if (a.node_count > r.cap) {
    for (void** p : {(void**)&r.d_flags, (void**)&r.d_cbox}) { if (*p) BR_TRY(hipFree(*p)); *p = nullptr; }
    r.cap = 0;
    const size_t cap = ((size_t)a.node_count + 1023) & ~(size_t)1023;
    BR_TRY(hipMalloc((void**)&r.d_flags, cap * sizeof(uint32_t)));
    BR_TRY(hipMalloc((void**)&r.d_cbox, cap * 12 * sizeof(float)));
    r.cap = cap;
  }
  const hipStream_t s = a.stream;
  float* verts = a.d_verts + a.first_float;
  if (a.d_src) {
    // the caller's vertices, read in the caller's stream order; from here on the caller may overwrite its buffer
    BR_TRY(hipMemcpyAsync(verts, a.d_src, (size_t)a.span_floats * sizeof(float), hipMemcpyDeviceToDevice, a.src_stream));
    if (a.src_stream != s) {
      BR_TRY(hipEventRecord(r.ev_in, a.src_stream));
      BR_TRY(hipStreamWaitEvent(s, r.ev_in, 0));
    }
  }
  BvhNodeQ* nodes = a.d_nodes + a.node_base;
  int32_t* parent = r.d_parent + a.node_base;
  const unsigned nb = (a.node_count + 255u) / 256u;
  const uint32_t nv = a.span_floats / 6u;
  const bool timed = getenv("RT_BUILD_TIMING") != nullptr;
  if (timed) {
    if (!r.ev_t0) BR_TRY(hipEventCreate(&r.ev_t0));
    if (!r.ev_t1) BR_TRY(hipEventCreate(&r.ev_t1));
    BR_TRY(hipEventRecord(r.ev_t0, s));
  }
  BR_TRY(hipMemsetAsync(r.d_sum, 0, sizeof(RefitSummary), s));
  BR_TRY(hipMemsetAsync(r.d_flags, 0, (size_t)a.node_count * sizeof(uint32_t), s));
  if (a.derive_parents) {
    BR_TRY(hipMemsetAsync(parent, 0xFF, (size_t)a.node_count * sizeof(int32_t), s));   // PARENT_ROOT until a node claims the slot
    hipLaunchKernelGGL(k_refit_parents, dim3(nb), dim3(256), 0, s, nodes, a.node_count, a.node_base, parent, r.d_sum);
  }
  if (nv) hipLaunchKernelGGL(k_refit_check, dim3((nv + 255u) / 256u), dim3(256), 0, s, verts, nv, r.d_sum);
  hipLaunchKernelGGL(k_refit_leaves, dim3(nb), dim3(256), 0, s, nodes, a.node_count, parent, verts, a.span_floats, a.d_idx + a.first_index, a.prim_count,
                     a.d_tris, a.tri_base, r.d_cbox, r.d_flags, r.d_sum);
  hipLaunchKernelGGL(k_refit_quant, dim3(1), dim3(64), 0, s, r.d_sum, a.d_mesh_entry);
  hipLaunchKernelGGL(k_refit_emit, dim3(nb), dim3(256), 0, s, nodes, a.node_count, parent, r.d_cbox, r.d_sum);
  if (a.cover_count)
    hipLaunchKernelGGL(k_refit_cover, dim3((a.cover_count + 255u) / 256u), dim3(256), 0, s, a.d_nodes, a.node_base, a.node_base + (int32_t)a.node_count,
                       a.d_cover_src + a.cover_first, a.cover_count, r.d_sum, a.d_cover_boxes + 6ull * a.cover_first);
  BR_TRY(hipGetLastError());
  if (timed) BR_TRY(hipEventRecord(r.ev_t1, s));
  BR_TRY(hipMemcpyAsync(r.h_sum, r.d_sum, sizeof(RefitSummary), hipMemcpyDeviceToHost, s));
  BR_TRY(hipStreamSynchronize(s));
  if (timed) {
    float ms = 0.f;
    BR_TRY(hipEventElapsedTime(&ms, r.ev_t0, r.ev_t1));
    fprintf(stderr, "[blas_refit] %u node slots, %u triangles, %s: kernels %.4f ms\n", a.node_count, a.prim_count, a.derive_parents ? "parents derived" : "parents kept", ms);
  }
  return 0;
#undef BR_TRY
}

}  // namespace rt
