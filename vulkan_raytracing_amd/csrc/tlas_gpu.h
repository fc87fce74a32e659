// tlas_gpu.h — the TLAS built and refitted on the device from device-resident instance records (rt_set_instances_device;
// the reference's createTLAS over a device instance buffer, src/main.cpp:538-793), see tlas_gpu.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "rt_device.h"

namespace rt {

// One entry per mesh of a scene: what k_inst_records copies into an InstanceDev (the fields set_instances_frames takes from
// rt_api.cpp's Mesh), uploaded whenever the BLAS are linked.
struct TlasMeshDev {
  int32_t blas_root, blas_root4;
  uint32_t first_float, first_index;
  uint32_t cover_first, cover_count;
  uint32_t prim_count, built;
  int32_t levels;        // interior levels of the mesh's BVH2 (traversal stack)
  float q_lo[3], q_scale[3];
  float lo[3], hi[3];    // object-space bounds (instance world boxes)
};

// What one build or refit reports back to the host (a single readback).
struct TlasSummary {
  uint32_t bad_mesh;      // lowest instance index with an unknown mesh, 0xFFFFFFFF: none
  uint32_t unbuilt;       // lowest instance index whose mesh has no BLAS, 0xFFFFFFFF: none
  uint32_t far;           // some instance's object-space test fails at a corner of G (far_possible, rt_api.cpp)
  int32_t depth;          // deepest leaf of the TLAS (interior nodes above it)
  int32_t blas_levels;    // deepest BLAS any instance enters
  uint32_t bounds[6];     // world bounds of the instance boxes (ordered-float lo[3], hi[3])
  uint32_t cbounds[6];    // bounds of their centroids (Morton codes)
  float q_lo[3], q_scale[3];   // the TLAS dequantisation (quant_params over `bounds`)
};

// Grow-only scratch and topology of one context's device TLAS.
struct TlasGpu {
  hipStream_t stream = nullptr;   // build stream: waits for the caller's stream, never for the context's frames
  hipEvent_t ev_in = nullptr;
  void* d_rec = nullptr;          // the library's copy of the caller's rt_instance records (re-issued by rt_set_instance_types)
  float* d_boxes = nullptr;       // instance world boxes (6 floats each)
  uint32_t *d_keys = nullptr, *d_keys2 = nullptr, *d_vals = nullptr, *d_vals2 = nullptr;   // Morton codes / instance ids, sorted: d_*2
  void* d_sort_tmp = nullptr;
  size_t sort_bytes = 0;
  int2* d_children = nullptr; int2* d_ranges = nullptr;
  int *d_parent_int = nullptr, *d_parent_leaf = nullptr, *d_height = nullptr;
  float* d_node_boxes = nullptr;
  uint32_t* d_flags = nullptr;
  uint32_t* d_types = nullptr;    // rt_set_instance_types table
  size_t types_cap = 0;
  TlasSummary* d_sum = nullptr;
  TlasSummary* h_sum = nullptr;   // pinned
  size_t cap = 0;                 // instances the scratch holds
  int topo_n = 0;                 // instances of the topology in d_children / d_parent_* / d_vals2 (0: none, refit impossible)
};

struct TlasBuildArgs {
  const void* d_src;        // caller's records (device); copied into d_rec on src_stream unless it IS d_rec
  hipStream_t src_stream;
  int n;
  bool refit;               // keep the topology of the last build (topo_n == n), recompute boxes bottom-up
  const TlasMeshDev* meshes; int n_meshes;
  const uint32_t* h_types; int n_types;   // host table (uploaded on the build stream), n_types == 0: TYPE_BY_OBJECT_INDEX
  InstanceDev* d_inst;      // records of the target parity
  BvhNodeQ* d_nodes;        // first node of the target parity's TLAS region; max(1, n - 1) nodes are written
  int32_t node_base;        // global index of d_nodes[0] (interior links are rebased to it)
};

// Enqueues the build (or refit) on g.stream, reads the summary back into *g.h_sum and waits for it (the reference also
// waits on its fence inside createTLAS, src/main.cpp:772-778).  Returns 0, or 1 with err set on a HIP error.
int tlas_gpu_build(TlasGpu& g, const TlasBuildArgs& a, std::string& err);
void tlas_gpu_free(TlasGpu& g);

}  // namespace rt
