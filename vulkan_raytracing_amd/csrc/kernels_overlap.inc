// kernels_overlap.inc — included by kernels.hip after walk_overlap.inc (product and alt translation units alike).
// rt_overlap_boxes_device: for every query box the triangles of the scene that touch it — their number and the smallest of them by
// (inst, prim).  The box shape of the overlap family (walk_overlap.inc: the walk, the row, the pruning, the node test), one lane per box:
//
//  * the record is 32 bytes, (lo.xyz, w3), (hi.xyz, w7): valid when every coordinate is finite and lo <= hi; its bounds are the box;
//  * the triangle test is the canonical sequence of DESIGN.md §5 in world space (overlap_tri): it depends on the box, the instance
//    record and the packet only, so the candidate set is the same whatever the tree.

// the smallest projection beyond the radius or the largest below its negative (strict: a tie is not a separation; fminf / fmaxf:
// a NaN among numbers is passed over, three NaNs separate nothing).  The predicate is evaluated without branches, every axis of it.
__device__ __forceinline__ bool axis_separates(float p0, float p1, float p2, float r) {
  const bool above = fminf(fminf(p0, p1), p2) > r, below = fmaxf(fmaxf(p0, p1), p2) < -r;
  return above | below;
}
// the three axes e_x x f, e_y x f, e_z x f of one edge f against the centred triangle (v0, v1, v2) and the half extent h
__device__ __forceinline__ bool edge_separates(F3 f, F3 v0, F3 v1, F3 v2, F3 h) {
  const F3 af = mk3(__builtin_fabsf(f.x), __builtin_fabsf(f.y), __builtin_fabsf(f.z));
  const bool sx = axis_separates(v0.z * f.y - v0.y * f.z, v1.z * f.y - v1.y * f.z, v2.z * f.y - v2.y * f.z, h.y * af.z + h.z * af.y);
  const bool sy = axis_separates(v0.x * f.z - v0.z * f.x, v1.x * f.z - v1.z * f.x, v2.x * f.z - v2.z * f.x, h.x * af.z + h.z * af.x);
  const bool sz = axis_separates(v0.y * f.x - v0.x * f.y, v1.y * f.x - v1.x * f.y, v2.y * f.x - v2.x * f.y, h.x * af.y + h.y * af.x);
  return sx | sy | sz;
}
// The canonical triangle-against-box test (DESIGN.md §5 "Box overlaps"): Akenine-Möller's 13 axes in binary32 and in world space.
// A, ab, ac: the packet through the instance's o2w.  True: nothing separates the pair (a candidate).
__device__ __forceinline__ bool overlap_tri(F3 lo, F3 hi, F3 A, F3 ab, F3 ac) {
  const F3 B = add3(A, ab), C = add3(A, ac);
  const bool finite = finite_bits(A.x) && finite_bits(A.y) && finite_bits(A.z) && finite_bits(B.x) && finite_bits(B.y) && finite_bits(B.z) &&
                      finite_bits(C.x) && finite_bits(C.y) && finite_bits(C.z);
  // the box axes, on lo / hi themselves
  bool sep = (fminf(fminf(A.x, B.x), C.x) > hi.x) || (fmaxf(fmaxf(A.x, B.x), C.x) < lo.x) || (fminf(fminf(A.y, B.y), C.y) > hi.y) ||
             (fmaxf(fmaxf(A.y, B.y), C.y) < lo.y) || (fminf(fminf(A.z, B.z), C.z) > hi.z) || (fmaxf(fmaxf(A.z, B.z), C.z) < lo.z);
  if (sep || !finite) return false;   // (most packets of a leaf end here)
  const F3 c = mk3(0.5f * lo.x + 0.5f * hi.x, 0.5f * lo.y + 0.5f * hi.y, 0.5f * lo.z + 0.5f * hi.z);
  const F3 h = mk3(0.5f * hi.x - 0.5f * lo.x, 0.5f * hi.y - 0.5f * lo.y, 0.5f * hi.z - 0.5f * lo.z);
  const F3 v0 = sub3(A, c), v1 = sub3(B, c), v2 = sub3(C, c);
  const F3 f0 = sub3(v1, v0), f1 = sub3(v2, v1), f2 = sub3(v0, v2);
  const bool s0 = edge_separates(f0, v0, v1, v2, h), s1 = edge_separates(f1, v0, v1, v2, h), s2 = edge_separates(f2, v0, v1, v2, h);
  sep = s0 | s1 | s2;
  const F3 n = cross3(f0, f1);
  const float d = dot3(n, v0), r = dot3(h, mk3(__builtin_fabsf(n.x), __builtin_fabsf(n.y), __builtin_fabsf(n.z)));
  return !(sep | (__builtin_fabsf(d) > r));
}

struct OverlapBox {
  __device__ __forceinline__ static bool load(const OverlapArgs& a, uint32_t bx, F3& wlo, F3& whi, float& mag, int& against) {
    const float4 r0 = ld_stream(&a.records[2u * (size_t)bx]), r1 = ld_stream(&a.records[2u * (size_t)bx + 1u]);
    wlo = mk3(r0.x, r0.y, r0.z); whi = mk3(r1.x, r1.y, r1.z);
    const bool valid = finite_bits(r0.x) && finite_bits(r0.y) && finite_bits(r0.z) && finite_bits(r1.x) && finite_bits(r1.y) && finite_bits(r1.z) &&
                       r0.x <= r1.x && r0.y <= r1.y && r0.z <= r1.z;
    mag = fmaxf(fmaxf(fmaxf(__builtin_fabsf(r0.x), __builtin_fabsf(r0.y)), __builtin_fabsf(r0.z)),
                fmaxf(fmaxf(__builtin_fabsf(r1.x), __builtin_fabsf(r1.y)), __builtin_fabsf(r1.z)));
    against = -1;   // (no by-reference form)
    return valid;
  }
  using Item = NoItem;
  struct Leaf {   // (the bounds are the whole record)
    __device__ __forceinline__ Leaf(const OverlapArgs&, uint32_t, const Item&) {}
    __device__ __forceinline__ bool touches(F3 wlo, F3 whi, F3 A, F3 ab, F3 ac) const { return overlap_tri(wlo, whi, A, ab, ac); }
  };
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_overlap_boxes(OverlapArgs a) { overlap_body<OverlapBox, false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_overlap_boxes_count(OverlapArgs a) { overlap_body<OverlapBox, true>(a); }
