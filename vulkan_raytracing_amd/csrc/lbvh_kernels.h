// lbvh_kernels.h — the LBVH front end shared by the BLAS builder (bvh_gpu.hip) and the device TLAS builder (tlas_gpu.hip):
// ordered-float bounds, 30-bit Morton codes of box centroids, the binary radix tree over the sorted codes (Karras, "Maximizing
// Parallelism in the Construction of BVHs, Octrees, and k-d Trees", HPG 2012) and box helpers.  Everything sits in an anonymous
// namespace: each TU that includes the header gets its own copy of the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace rt {
namespace {

// monotone float <-> uint mapping so that atomicMin/atomicMax on uints order floats
__device__ __forceinline__ uint32_t f2ord(float f) { uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float ord2f(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

struct Box { float lo[3], hi[3]; };

__global__ void k_init_bounds(uint32_t* b) {
  if (threadIdx.x < 3) b[threadIdx.x] = 0xFFFFFFFFu;       // min accumulators
  else if (threadIdx.x < 6) b[threadIdx.x] = 0u;           // max accumulators
}

__device__ __forceinline__ uint32_t spread3(uint32_t v) {   // 10 bits -> every third bit
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}

__global__ __launch_bounds__(256) void k_morton(const Box* boxes, uint32_t n, const uint32_t* cbounds, uint32_t* keys, uint32_t* vals) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  uint32_t code = 0;
  for (int k = 0; k < 3; k++) {
    const float lo = ord2f(cbounds[k]), hi = ord2f(cbounds[3 + k]);
    const float ext = hi - lo;
    const float cen = 0.5f * boxes[p].lo[k] + 0.5f * boxes[p].hi[k];
    float t = ext > 0.f ? (cen - lo) / ext : 0.f;
    t = fminf(fmaxf(t * 1024.0f, 0.0f), 1023.0f);
    code |= spread3((uint32_t)t) << (2 - k);
  }
  keys[p] = code; vals[p] = p;
}

// common-prefix length of sorted keys i and j (ties broken by the index), -1 outside the array
__device__ __forceinline__ int delta(const uint32_t* keys, int n, int i, int j) {
  if (j < 0 || j >= n) return -1;
  const uint32_t a = keys[i], b = keys[j];
  if (a == b) return 32 + __clz((uint32_t)i ^ (uint32_t)j);
  return __clz(a ^ b);
}

// One thread per internal node i in [0, n-1): range, split, children, parents (Karras 2012, algorithm 1).
// child encoding here: >= 0 internal node, < 0 leaf ~sorted_index
__global__ __launch_bounds__(256) void k_radix_tree(const uint32_t* keys, int n, int2* children, int2* ranges, int* parent_internal, int* parent_leaf) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n - 1) return;
  const int d = (delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
  const int dmin = delta(keys, n, i, i - d);
  int lmax = 2;
  while (delta(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
  int l = 0;
  for (int t = lmax >> 1; t >= 1; t >>= 1)
    if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
  const int j = i + l * d;
  const int dnode = delta(keys, n, i, j);
  int s = 0;
  for (int t = (l + 1) >> 1;; t = (t + 1) >> 1) {
    if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    if (t <= 1) break;
  }
  const int gamma = i + s * d + min(d, 0);
  const int lo = min(i, j), hi = max(i, j);
  const int left = (lo == gamma) ? ~gamma : gamma;
  const int right = (hi == gamma + 1) ? ~(gamma + 1) : (gamma + 1);
  children[i] = make_int2(left, right);
  ranges[i] = make_int2(lo, hi);
  if (left >= 0) parent_internal[left] = i; else parent_leaf[~left] = i;
  if (right >= 0) parent_internal[right] = i; else parent_leaf[~right] = i;
  if (i == 0) parent_internal[0] = -1;
}

__device__ __forceinline__ Box box_union(const Box& a, const Box& b) {
  Box m;
  for (int k = 0; k < 3; k++) { m.lo[k] = fminf(a.lo[k], b.lo[k]); m.hi[k] = fmaxf(a.hi[k], b.hi[k]); }
  return m;
}
__device__ __forceinline__ float box_half_area(const Box& b) {
  const float dx = b.hi[0] - b.lo[0], dy = b.hi[1] - b.lo[1], dz = b.hi[2] - b.lo[2];
  return dx * dy + dy * dz + dz * dx;
}

}  // namespace
}  // namespace rt
