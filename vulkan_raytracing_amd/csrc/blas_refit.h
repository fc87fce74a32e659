// blas_refit.h — a mesh's BLAS refitted on the device from new vertex positions (rt_refit_blas_device; Vulkan's BLAS update,
// mode = UPDATE over a device vertex buffer), see blas_refit.hip.  The tree topology and the linked layout stay; packets, boxes,
// quantisation, the mesh-table entry and the frontier boxes are recomputed in place in the scene's linked arrays.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "rt_device.h"
#include "tlas_gpu.h"

namespace rt {

// What one refit reports back to the host (a single readback).
struct RefitSummary {
  float root_lo[3], root_hi[3];   // the new root box (Mesh::bounds)
  float q_lo[3], q_scale[3];      // the new dequantisation of the mesh's planes
  uint32_t nonfinite;             // some position of the vertex span is not finite
  uint32_t bad;                   // a link or a leaf range outside the mesh (never for a tree link_blas produced)
  uint32_t root_done;             // the climb reached the root
  uint32_t pad;
};

// Scene-wide refit state, grow-only and kept between calls.
struct BlasRefitScratch {
  hipEvent_t ev_in = nullptr;     // the caller's copy is done (its stream -> the refit stream)
  hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;   // RT_BUILD_TIMING: around the refit's kernels
  int32_t* d_parent = nullptr;    // per linked node slot: (parent's local slot << 1) | child, -1 root, -2 filler; valid per mesh (Mesh::parents_ready)
  size_t parent_cap = 0;
  uint32_t* d_flags = nullptr;    // per slot of the refitted mesh: arrival count of the climb
  float* d_cbox = nullptr;        // per slot: the float boxes of its two children (12 floats)
  size_t cap = 0;                 // slots d_flags / d_cbox hold
  RefitSummary* d_sum = nullptr;
  RefitSummary* h_sum = nullptr;  // pinned
};

struct BlasRefitArgs {
  const float* d_src;           // caller's vertices (span_floats floats), copied into d_verts + first_float on src_stream; NULL: refit from d_verts as it is
  hipStream_t src_stream;
  hipStream_t stream;           // the refit's kernels and the readback
  float* d_verts; const uint32_t* d_idx;   // the scene's vertex / index buffers
  uint32_t first_float, first_index, span_floats, prim_count;
  BvhNodeQ* d_nodes;            // the scene's linked node array
  int32_t node_base; uint32_t node_count;  // the mesh's slots [node_base, node_base + node_count) (treelet layout, root first)
  float4* d_tris; uint32_t tri_base;       // the linked packets; the mesh's are [tri_base, tri_base + prim_count)
  const uint32_t* d_cover_src;  // per frontier box of the scene: (parent node << 1) | child, the cut link_blas chose
  float* d_cover_boxes; uint32_t cover_first, cover_count;
  TlasMeshDev* d_mesh_entry;    // the mesh's entry of the scene's mesh table
  bool derive_parents;          // first refit of the mesh since it was linked
};

// Grows d_parent to n_slots (the scene's linked BLAS part); *grown tells that the kept parents are gone.
int blas_refit_reserve(BlasRefitScratch& r, size_t n_slots, bool* grown, std::string& err);
// Enqueues the refit on a.stream, reads the summary back into *r.h_sum and waits for it.  Returns 0, or 1 with err set on a HIP error.
// With RT_BUILD_TIMING set, the time of the refit's kernels (HIP events on a.stream, the caller's copy excluded) goes to stderr.
int blas_refit(BlasRefitScratch& r, const BlasRefitArgs& a, std::string& err);
void blas_refit_free(BlasRefitScratch& r);

}  // namespace rt
