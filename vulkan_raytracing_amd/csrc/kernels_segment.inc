// kernels_segment.inc — included by kernels.hip after kernels_inside.inc (product and alt translation units alike).
// rt_closest_segment_device: for every segment record (P0, r_max, P1) the nearest pair of a point of the closed segment P0..P1 and a
// point of the scene's surface within the record's radius.  The segment shape of the nearest-pair family (walk_nearest.inc), one lane
// per segment:
//
//  * the segment is held as its midpoint m and half vector h in the space of the tree being walked: in world space for TLAS nodes, in
//    the instance's object space for BLAS nodes (both endpoints through w2o);
//  * node test (i): the per-axis gap |m - c| - e - |h| between the segment's interval and the box (centre c, half extents e), every axis
//    shortened by the family's absolute slack (the magnitudes: both endpoints, the planes, the rows of the transforms, word 0 of
//    k_closest_scale's array), the sum of squares times 1 - 2^-13 (DESIGN.md §5 "Closest points of segments"); it orders the children;
//  * node test (ii) (RT_SEGMENT_SLAB): the slab test of the path m + s h, s in [-1, 1], against the box inflated on every side by
//    rho = sqrt(best / scale2) (1 + 2^-13) plus the same slack, in its separating-axis form (Ericson, Real-Time Collision Detection
//    §5.3.3): the three box axes are test (i), the three axes cross(axis, h) are tested here, without a reciprocal direction.  A
//    segment within rho of a box meets the box inflated by rho on every side.  An unbounded best (rho = +inf) or a NaN opens the box;
//  * the triangle test is the canonical sequence of DESIGN.md §5 in world space (segment_tri); the result word is the parameter s.
#ifndef RT_SEGMENT_WAVES_PER_EU
#define RT_SEGMENT_WAVES_PER_EU 4   /* the record-level walks' budget */
#endif
#ifndef RT_SEGMENT_SLAB
#define RT_SEGMENT_SLAB 1           /* node test (ii); 0: test (i) alone (tools/closest_segment_cost.py measures both) */
#endif

// the canonical clamp to [0, 1]: NaN and -0 give +0 (fminf(fmaxf(x, 0), 1) with the sign of a zero result fixed)
__device__ __forceinline__ float seg_clamp(float x) { return x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f; }

// The canonical nearest pair of the segment P0..P1 and the triangle (a, ab, ac), the packet through the instance's o2w (DESIGN.md §5
// "Closest points of segments"): binary32, world space.  Every feature proposes a point pair and its d2 is the distance computed
// between the two: the closest-point sequence for P0, P1 and (when the endpoints lie strictly on both sides of the plane) the plane
// crossing X, then Ericson §5.1.9 for the edges AB, AC, BC with exact-zero tests.  A later feature replaces an earlier one only when
// its d2 is strictly smaller; a NaN d2 is skipped.  Returns d2 (NaN: no feature, never a candidate), (u, v) of B and C, and s.
// Two loops that stay loops: five closest-point-sized features side by side do not fit the register budget.
__device__ __forceinline__ float segment_tri(F3 P0, F3 P1, F3 a, F3 ab, F3 ac, float& u, float& v, float& s) {
  const F3 d = sub3(P1, P0);
  const bool point = P0.x == P1.x && P0.y == P1.y && P0.z == P1.z;   // answered by the first feature alone: rt_closest_point_device's record
  float best = __builtin_nanf("");
  u = 0.0f; v = 0.0f; s = 0.0f;
  const int n_points = point ? 1 : 3;
#pragma unroll 1
  for (int k = 0; k < n_points; k++) {
    F3 p = P0;
    float sk = 0.0f;
    if (k == 1) { p = P1; sk = 1.0f; }
    if (k == 2) {
      const F3 n = cross3(ab, ac);
      const float h0 = dot3(n, sub3(P0, a)), h1 = dot3(n, sub3(P1, a));
      if (!((h0 < 0.0f && h1 > 0.0f) || (h0 > 0.0f && h1 < 0.0f))) break;
      sk = seg_clamp(h0 / (h0 - h1));
      p = mk3(P0.x + sk * d.x, P0.y + sk * d.y, P0.z + sk * d.z);
    }
    float uu, vv;
    const float d2 = closest_tri(p, a, ab, ac, uu, vv);
    if (d2 == d2 && !(d2 >= best)) { best = d2; u = uu; v = vv; s = sk; }
  }
  if (point) return best;
  const float A = dot3(d, d);
#pragma unroll 1
  for (int k = 0; k < 3; k++) {
    const F3 q = k == 2 ? mk3(a.x + ab.x, a.y + ab.y, a.z + ab.z) : a;
    const F3 e = k == 0 ? ab : (k == 1 ? ac : sub3(ac, ab));
    const F3 r = sub3(P0, q);
    const float E = dot3(e, e), Fq = dot3(e, r), C = dot3(d, r), B = dot3(d, e);
    float ss = 0.0f, tt = 0.0f;
    if (A == 0.0f && E == 0.0f) { }
    else if (A == 0.0f) tt = seg_clamp(Fq / E);
    else if (E == 0.0f) ss = seg_clamp(-C / A);
    else {
      const float denom = A * E - B * B;
      ss = denom != 0.0f ? seg_clamp((B * Fq - C * E) / denom) : 0.0f;
      tt = (B * ss + Fq) / E;
      if (tt < 0.0f) { tt = 0.0f; ss = seg_clamp(-C / A); }
      else if (tt > 1.0f) { tt = 1.0f; ss = seg_clamp((B - C) / A); }
    }
    const F3 w = mk3((P0.x + ss * d.x) - (q.x + tt * e.x), (P0.y + ss * d.y) - (q.y + tt * e.y), (P0.z + ss * d.z) - (q.z + tt * e.z));
    const float d2 = dot3(w, w);
    if (d2 == d2 && !(d2 >= best)) {
      best = d2; s = ss;
      u = k == 0 ? tt : (k == 1 ? 0.0f : 1.0f - tt);
      v = k == 0 ? 0.0f : tt;
    }
  }
  return best;
}

// Node tests (i) and (ii) of the quantised box (wx, wy, wz) of a tree with dequantisation (q_lo, q_scale) against the segment m +- h.
// b: the deflated squared gap of test (i) (every axis gap shortened by `slack`, the sum times `scale2`).  True: the box is open — b does
// not exceed best and (RT_SEGMENT_SLAB) no axis cross(axis, h) separates the path from the box inflated by slack + rho.  Comparisons
// are written so that a NaN opens the box.
__device__ __forceinline__ bool segment_box(uint32_t wx, uint32_t wy, uint32_t wz, F3 m, F3 h, F3 q_lo, F3 q_scale, float slack, float scale2, float rho,
                                            float best, float& b) {
  F3 lo, hi;
  box_planes(wx, wy, wz, q_lo, q_scale, lo, hi);
  const float ex = (hi.x - lo.x) * 0.5f, ey = (hi.y - lo.y) * 0.5f, ez = (hi.z - lo.z) * 0.5f;
  const float mx = m.x - (lo.x + hi.x) * 0.5f, my = m.y - (lo.y + hi.y) * 0.5f, mz = m.z - (lo.z + hi.z) * 0.5f;
  const float ahx = __builtin_fabsf(h.x), ahy = __builtin_fabsf(h.y), ahz = __builtin_fabsf(h.z);
  const float gx = fmaxf(((__builtin_fabsf(mx) - ex) - ahx) - slack, 0.0f);
  const float gy = fmaxf(((__builtin_fabsf(my) - ey) - ahy) - slack, 0.0f);
  const float gz = fmaxf(((__builtin_fabsf(mz) - ez) - ahz) - slack, 0.0f);
  b = (gx * gx + gy * gy + gz * gz) * scale2;
  bool open = !(b > best);   // (inclusive, and an unbounded best opens all)
#if RT_SEGMENT_SLAB
  const float infl = slack + rho;
  const float fx = ex + infl, fy = ey + infl, fz = ez + infl;
  const bool sep = __builtin_fabsf(my * h.z - mz * h.y) > fy * ahz + fz * ahy || __builtin_fabsf(mz * h.x - mx * h.z) > fz * ahx + fx * ahz ||
                   __builtin_fabsf(mx * h.y - my * h.x) > fx * ahy + fy * ahx;
  open = open && !sep;
#endif
  return open;
}

struct NearestSegment {
  static constexpr uint32_t STRIDE = 2;
  struct Params { float s = 0.f; };           // the segment's point of the nearest pair
  F3 w0 = mk3(0, 0, 0), w1 = w0;              // the endpoints in world space
  F3 m = w0, h = w0;                          // midpoint and half vector in the space of the tree being walked
  float rho = 0.f;                            // the reach of the best d2 in that space's units, rounded up
  __device__ __forceinline__ bool load(const NearestArgs& a, uint32_t pt, float& r_max, float& pmag, int& against) {
    const float4 r0 = ld_stream(&a.records[2u * (size_t)pt]), r1 = ld_stream(&a.records[2u * (size_t)pt + 1u]);
    w0 = mk3(r0.x, r0.y, r0.z); w1 = mk3(r1.x, r1.y, r1.z); r_max = r0.w; against = -1;
    pmag = fmaxf(fmaxf(fmaxf(__builtin_fabsf(r0.x), __builtin_fabsf(r0.y)), __builtin_fabsf(r0.z)),
                 fmaxf(fmaxf(__builtin_fabsf(r1.x), __builtin_fabsf(r1.y)), __builtin_fabsf(r1.z)));
    return finite_bits(r0.x) && finite_bits(r0.y) && finite_bits(r0.z) && finite_bits(r1.x) && finite_bits(r1.y) && finite_bits(r1.z) && r0.w >= 0.0f;
  }
  __device__ __forceinline__ void hold(F3 p0, F3 p1) {
    m = mk3(p0.x * 0.5f + p1.x * 0.5f, p0.y * 0.5f + p1.y * 0.5f, p0.z * 0.5f + p1.z * 0.5f);
    h = mk3(p1.x * 0.5f - p0.x * 0.5f, p1.y * 0.5f - p0.y * 0.5f, p1.z * 0.5f - p0.z * 0.5f);
  }
  __device__ __forceinline__ void to_world() { hold(w0, w1); }
  __device__ __forceinline__ F3 enter(const InstanceDev* I) {
    hold(xform_point(I->w2o, w0), xform_point(I->w2o, w1));
    return mk3(fmaxf(__builtin_fabsf(w0.x), __builtin_fabsf(w1.x)), fmaxf(__builtin_fabsf(w0.y), __builtin_fabsf(w1.y)), fmaxf(__builtin_fabsf(w0.z), __builtin_fabsf(w1.z)));
  }
  __device__ __forceinline__ void reach(float best, float scale2) { rho = __builtin_sqrtf(best / scale2) * SW_T_HI; }
  __device__ __forceinline__ bool open(uint32_t wx, uint32_t wy, uint32_t wz, F3 q_lo, F3 q_scale, float slack, float scale2, float best, float& b) const {
    return segment_box(wx, wy, wz, m, h, q_lo, q_scale, slack, scale2, rho, best, b);
  }
  __device__ __forceinline__ float test(F3 a, F3 ab, F3 ac, float& u, float& v, Params& p) const { return segment_tri(w0, w1, a, ab, ac, u, v, p.s); }
  __device__ __forceinline__ static void store(const NearestArgs& a, uint32_t pt, Params p) {
    if (a.params) a.params[pt] = p.s;
  }
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_SEGMENT_WAVES_PER_EU))) void k_closest_segment(NearestArgs a) { nearest_body<NearestSegment, false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_SEGMENT_WAVES_PER_EU))) void k_closest_segment_count(NearestArgs a) { nearest_body<NearestSegment, true>(a); }

// The side of the reported triangle's plane the segment's point of the nearest pair lies on, into word 7 of its rt_hit_attr (after
// k_hit_attr): k_closest_side's rule at p = P0 + s d, d = P1 - P0 (per component one product and one sum), 0 on a miss.
__global__ __launch_bounds__(256) void k_segment_side(SceneDev sc, const float4* __restrict__ segs, const float* __restrict__ params, const HitRec* __restrict__ hits,
                                                     uint32_t* __restrict__ attr, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const HitRec hr = hits[i];
  uint32_t kind = 0u;
  if (hr.inst >= 0) {
    const float4 r0 = segs[2u * (size_t)i], r1 = segs[2u * (size_t)i + 1u];
    const float s = params[i];
    const float4 p = make_float4(r0.x + s * (r1.x - r0.x), r0.y + s * (r1.y - r0.y), r0.z + s * (r1.z - r0.z), 0.0f);
    kind = closest_side_word(sc, &p, hr);
  }
  attr[8u * (size_t)i + 7u] = kind;
}

void launch_segment_side(const SceneDev& sc, const float4* segs, const float* params, const HitRec* hits, float4* attr, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_segment_side, dim3((n + 255u) / 256u), dim3(256), 0, s, sc, segs, params, hits, reinterpret_cast<uint32_t*>(attr), n);
}
