// kernels_triangles.inc — included by kernels.hip after kernels_overlap.inc (product and alt translation units alike).
// rt_overlap_triangles_device: for every query triangle the triangles of the scene that cut or touch it — their number and the smallest
// of them by (inst, prim).  The triangle shape of the overlap family (walk_overlap.inc), one lane per query triangle:
//
//  * the record is 48 bytes, (P0.xyz, w3), (P1.xyz, w7), (P2.xyz, w11): valid when every coordinate is finite; its bounds are
//    [min(P0, P1, P2), max(P0, P1, P2)], so the walk visits the nodes and packets k_overlap_boxes visits for the bounding boxes;
//  * the triangle test is the canonical sequence of DESIGN.md §5 "Triangle overlaps" in world space (collide_tri): the bounds of the
//    candidate against the bounds of the query, then seventeen separating axes on vertices centred on P0.  It depends on the query
//    record, the instance record and the packet only;
//  * the lane keeps the query's bounds across the walk and reads the 48-byte record again at every leaf (resident in cache): nine
//    floats fewer beside the walk state;
//  * by reference (kernels_refs.inc): words 7 and 11 are the source instance and `against`, read again at every TLAS leaf.

// one axis L: the query projects to 0, L.p1, L.p2 and the candidate to L.a, L.b, L.c (everything centred on P0).  Strict: a tie is not a
// separation; a zero axis projects everything to 0 and separates nothing; fminf / fmaxf pass over a NaN among numbers.
__device__ __forceinline__ bool collide_axis(F3 L, F3 p1, F3 p2, F3 a, F3 b, F3 c) {
  const float q1 = dot3(L, p1), q2 = dot3(L, p2), ta = dot3(L, a), tb = dot3(L, b), tc = dot3(L, c);
  const float qmin = fminf(fminf(0.0f, q1), q2), qmax = fmaxf(fmaxf(0.0f, q1), q2);
  const float tmin = fminf(fminf(ta, tb), tc), tmax = fmaxf(fmaxf(ta, tb), tc);
  return (qmin > tmax) | (qmax < tmin);
}

// The canonical triangle-against-triangle test (DESIGN.md §5 "Triangle overlaps"), binary32, world space, every axis evaluated.
// [wlo, whi]: the query's bounds; A, ab, ac: the packet through the instance's o2w.  True: nothing separates the pair (a candidate).
__device__ __forceinline__ bool collide_tri(F3 wlo, F3 whi, F3 P0, F3 P1, F3 P2, F3 A, F3 ab, F3 ac) {
  const F3 B = add3(A, ab), C = add3(A, ac);
  const bool finite = finite_bits(A.x) && finite_bits(A.y) && finite_bits(A.z) && finite_bits(B.x) && finite_bits(B.y) && finite_bits(B.z) &&
                      finite_bits(C.x) && finite_bits(C.y) && finite_bits(C.z);
  // step 2: the bounds of the query, on the vertices themselves
  bool sep = (fminf(fminf(A.x, B.x), C.x) > whi.x) || (fmaxf(fmaxf(A.x, B.x), C.x) < wlo.x) || (fminf(fminf(A.y, B.y), C.y) > whi.y) ||
             (fmaxf(fmaxf(A.y, B.y), C.y) < wlo.y) || (fminf(fminf(A.z, B.z), C.z) > whi.z) || (fmaxf(fmaxf(A.z, B.z), C.z) < wlo.z);
  if (sep || !finite) return false;   // (most packets of a leaf end here)
  const F3 p1 = sub3(P1, P0), p2 = sub3(P2, P0);
  const F3 a = sub3(A, P0), b = sub3(B, P0), c = sub3(C, P0);
  const F3 g0 = p1, g1 = sub3(p2, p1), g2 = p2;
  const F3 f0 = sub3(b, a), f1 = sub3(c, b), f2 = sub3(a, c);
  const F3 n = cross3(g0, g2), m = cross3(f0, f1);
  sep = collide_axis(n, p1, p2, a, b, c);
  sep |= collide_axis(m, p1, p2, a, b, c);
  sep |= collide_axis(cross3(g0, f0), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g0, f1), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g0, f2), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g1, f0), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g1, f1), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g1, f2), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g2, f0), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g2, f1), p1, p2, a, b, c);
  sep |= collide_axis(cross3(g2, f2), p1, p2, a, b, c);
  sep |= collide_axis(cross3(n, g0), p1, p2, a, b, c);
  sep |= collide_axis(cross3(n, g1), p1, p2, a, b, c);
  sep |= collide_axis(cross3(n, g2), p1, p2, a, b, c);
  sep |= collide_axis(cross3(m, f0), p1, p2, a, b, c);
  sep |= collide_axis(cross3(m, f1), p1, p2, a, b, c);
  sep |= collide_axis(cross3(m, f2), p1, p2, a, b, c);
  return !sep;
}

struct OverlapTriangle {
  __device__ __forceinline__ static bool load(const OverlapArgs& a, uint32_t bx, F3& wlo, F3& whi, float& mag, int& against) {
    const float4* qp = a.records + 3u * (size_t)bx;
    const float4 r0 = ld_stream(&qp[0]), r1 = ld_stream(&qp[1]), r2 = ld_stream(&qp[2]);
    wlo = mk3(fminf(fminf(r0.x, r1.x), r2.x), fminf(fminf(r0.y, r1.y), r2.y), fminf(fminf(r0.z, r1.z), r2.z));
    whi = mk3(fmaxf(fmaxf(r0.x, r1.x), r2.x), fmaxf(fmaxf(r0.y, r1.y), r2.y), fmaxf(fmaxf(r0.z, r1.z), r2.z));
    mag = fmaxf(fmaxf(fmaxf(__builtin_fabsf(wlo.x), __builtin_fabsf(wlo.y)), __builtin_fabsf(wlo.z)),
                fmaxf(fmaxf(__builtin_fabsf(whi.x), __builtin_fabsf(whi.y)), __builtin_fabsf(whi.z)));
    against = (int)__float_as_uint(r2.w);
    return finite_bits(r0.x) && finite_bits(r0.y) && finite_bits(r0.z) && finite_bits(r1.x) && finite_bits(r1.y) && finite_bits(r1.z) &&
           finite_bits(r2.x) && finite_bits(r2.y) && finite_bits(r2.z);
  }
  using Item = NoItem;
  struct Leaf {   // the record read again
    F3 P0, P1, P2;
    __device__ __forceinline__ Leaf(const OverlapArgs& a, uint32_t bx, const Item&) {
      const float4* qp = a.records + 3u * (size_t)bx;
      const float4 r0 = qp[0], r1 = qp[1], r2 = qp[2];
      P0 = mk3(r0.x, r0.y, r0.z); P1 = mk3(r1.x, r1.y, r1.z); P2 = mk3(r2.x, r2.y, r2.z);
    }
    __device__ __forceinline__ bool touches(F3 wlo, F3 whi, F3 A, F3 ab, F3 ac) const { return collide_tri(wlo, whi, P0, P1, P2, A, ab, ac); }
  };
  __device__ __forceinline__ static bool own(const OverlapArgs& a, uint32_t bx, int ii) {
    const float4* qp = a.records + 3u * (size_t)bx;
    return (int)__float_as_uint(qp[2].w) < 0 && ii == (int)__float_as_uint(qp[1].w);
  }
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_collide_triangles(OverlapArgs a) { overlap_body<OverlapTriangle, false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_collide_triangles_count(OverlapArgs a) { overlap_body<OverlapTriangle, true>(a); }
