// kernels_triangle.inc — included by kernels.hip after kernels_segment.inc (product and alt translation units alike).
// rt_closest_triangle_device: for every triangle record (P0, r_max, P1, w7, P2, w11) the nearest pair of a point of the closed triangle
// P0 P1 P2 and a point of the scene's surface within the record's radius.  The triangle shape of the nearest-pair family
// (walk_nearest.inc), one lane per record:
//
//  * the query triangle is held as the centre m and the half extents eq of its three vertices' bounds in the space of the tree being
//    walked: in world space for TLAS nodes, in the instance's object space for BLAS nodes (the three vertices through w2o);
//  * node test (i): the per-axis gap |m - c| - e - eq between the triangle's bounds and the box (centre c, half extents e), every axis
//    shortened by the family's absolute slack, the sum of squares times 1 - 2^-13 (DESIGN.md §5 "Closest points of triangles"):
//    segment_box's test (i) with eq where it has |h|; it orders the children;
//  * node test (ii) (RT_TRIANGLE_PLANE): the query's plane against the box inflated on every side by rho = sqrt(best / scale2)
//    (1 + 2^-13) plus the same slack: with n_q = cross(P1 - P0, P2 - P0) in the walked space the box is skipped when
//    |dot(n_q, c - p0)| > sum_k (e_k + infl) |n_q,k| + E, E = 2^-17 L^3 (L the largest edge component) covering n_q's own rounding, so
//    that a needle's meaningless normal cannot prune.  An unbounded best (rho = +inf) or a NaN opens the box;
//  * the triangle test is the canonical sequence of DESIGN.md §5 in world space (triangle_tri); the result words are (qu, qv);
//  * by reference (kernels_refs.inc): words 7 and 11 are the source instance and `against`, read again at every TLAS leaf.
#ifndef RT_TRIANGLE_WAVES_PER_EU
#define RT_TRIANGLE_WAVES_PER_EU 4   /* the record-level walks' budget */
#endif
#ifndef RT_TRIANGLE_PLANE
#define RT_TRIANGLE_PLANE 1          /* node test (ii); 0: test (i) alone (tools/closest_triangle_cost.py measures both) */
#endif

// vertex k (0, 1, 2) of a triangle held in registers, by selects (the loops below stay loops)
__device__ __forceinline__ F3 tri_pick(int k, F3 p0, F3 p1, F3 p2) { return k == 0 ? p0 : (k == 1 ? p1 : p2); }

// Steps 1 and 2 (and, with the roles exchanged, 4 and 5) of the canonical sequence: the three points V0, V1, V2 and then the crossings
// of the edges (V[ea], V[eb]) with the plane of the triangle (a, ab, ac), each through closest_tri against that triangle.  For trip k
// the caller's `take(d2, k, s, tu, tv)` gets the feature's d2, the parameter s along the edge (crossings) and closest_tri's (u, v).
// edges: packed pairs of vertex numbers, two bits each, (ea, eb) of edge i in bits 4 i .. 4 i + 3.
template <class Take>
__device__ __forceinline__ void tri_points_and_crossings(F3 V0, F3 V1, F3 V2, uint32_t edges, F3 a, F3 ab, F3 ac, bool first_only, Take take) {
  const int trips = first_only ? 1 : 6;
#pragma unroll 1
  for (int k = 0; k < trips; k++) {
    F3 p;
    float sk = 0.0f;
    if (k < 3) p = tri_pick(k, V0, V1, V2);
    else {
      const uint32_t e = edges >> (4 * (k - 3));
      const F3 pi = tri_pick((int)(e & 3u), V0, V1, V2), pj = tri_pick((int)((e >> 2) & 3u), V0, V1, V2);
      const F3 n = cross3(ab, ac);
      const float h0 = dot3(n, sub3(pi, a)), h1 = dot3(n, sub3(pj, a));
      if (!((h0 < 0.0f && h1 > 0.0f) || (h0 > 0.0f && h1 < 0.0f))) continue;
      sk = seg_clamp(h0 / (h0 - h1));
      const F3 d = sub3(pj, pi);
      p = mk3(pi.x + sk * d.x, pi.y + sk * d.y, pi.z + sk * d.z);
    }
    float tu, tv;
    const float d2 = closest_tri(p, a, ab, ac, tu, tv);
    take(d2, k, sk, tu, tv);
  }
}

// The canonical nearest pair of the query triangle P0 P1 P2 and the scene triangle (a, ab, ac), the packet through the instance's o2w
// (DESIGN.md §5 "Closest points of triangles"): binary32, world space.  Every feature proposes a point pair and its d2 is the distance
// computed between the two.  In order: (1) the query's vertices on the scene triangle, (2) the query's edges crossing the scene
// triangle's plane, (3) the nine edge pairs (query-edge-major; segment_tri's edge block), (4) the scene's vertices on the query
// triangle, (5) the scene's edges crossing the query's plane.  A later feature replaces an earlier one only when its d2 is strictly
// smaller; a NaN d2 is skipped.  Returns d2 (NaN: no feature, never a candidate), (u, v) of B and C, and (qu, qv) of P1 and P2.
__device__ __forceinline__ float triangle_tri(F3 P0, F3 P1, F3 P2, F3 a, F3 ab, F3 ac, float& u, float& v, float& qu, float& qv) {
  const bool point = P0.x == P1.x && P0.y == P1.y && P0.z == P1.z && P0.x == P2.x && P0.y == P2.y && P0.z == P2.z;
  float best = __builtin_nanf("");
  u = 0.0f; v = 0.0f; qu = 0.0f; qv = 0.0f;
  // ---- 1, 2: query vertices and query edges (P0, P1), (P1, P2), (P2, P0) against the scene triangle
  tri_points_and_crossings(P0, P1, P2, 0x294u, a, ab, ac, point, [&](float d2, int k, float s, float tu, float tv) {
    if (d2 == d2 && !(d2 >= best)) {
      best = d2; u = tu; v = tv;
      // vertices: (0, 0), (1, 0), (0, 1); crossings: (s, 0), (1 - s, s), (0, 1 - s)
      qu = k == 1 ? 1.0f : (k == 3 ? s : (k == 4 ? 1.0f - s : 0.0f));
      qv = k == 2 ? 1.0f : (k == 4 ? s : (k == 5 ? 1.0f - s : 0.0f));
    }
  });
  if (point) return best;   // answered by the first feature alone: rt_closest_point_device's record
  // ---- 3: the nine edge pairs, query-edge-major, each scene edge AB, AC, BC (segment_tri's block for the segment Pi..Pj)
#pragma unroll 1
  for (int i = 0; i < 3; i++) {
    const F3 pi = tri_pick(i, P0, P1, P2), pj = tri_pick(i == 2 ? 0 : i + 1, P0, P1, P2);
    const F3 d = sub3(pj, pi);
    const float A = dot3(d, d);
#pragma unroll 1
    for (int k = 0; k < 3; k++) {
      const F3 q = k == 2 ? mk3(a.x + ab.x, a.y + ab.y, a.z + ab.z) : a;
      const F3 e = k == 0 ? ab : (k == 1 ? ac : sub3(ac, ab));
      const F3 r = sub3(pi, q);
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
      const F3 w = mk3((pi.x + ss * d.x) - (q.x + tt * e.x), (pi.y + ss * d.y) - (q.y + tt * e.y), (pi.z + ss * d.z) - (q.z + tt * e.z));
      const float d2 = dot3(w, w);
      if (d2 == d2 && !(d2 >= best)) {
        best = d2;
        u = k == 0 ? tt : (k == 1 ? 0.0f : 1.0f - tt);
        v = k == 0 ? 0.0f : tt;
        qu = i == 0 ? ss : (i == 1 ? 1.0f - ss : 0.0f);
        qv = i == 0 ? 0.0f : (i == 1 ? ss : 1.0f - ss);
      }
    }
  }
  // ---- 4, 5: scene vertices a, b, c and scene edges (a, b), (a, c), (b, c) against the query triangle (P0, g0, g2)
  const F3 b = mk3(a.x + ab.x, a.y + ab.y, a.z + ab.z), c = mk3(a.x + ac.x, a.y + ac.y, a.z + ac.z);
  tri_points_and_crossings(a, b, c, 0x984u, P0, sub3(P1, P0), sub3(P2, P0), false, [&](float d2, int k, float s, float tu, float tv) {
    if (d2 == d2 && !(d2 >= best)) {
      best = d2; qu = seg_clamp(tu); qv = seg_clamp(tv);
      // vertices: (0, 0), (1, 0), (0, 1); crossings: (s, 0), (0, s), (1 - s, s)
      u = k == 1 ? 1.0f : (k == 3 ? s : (k == 5 ? 1.0f - s : 0.0f));
      v = k == 2 ? 1.0f : (k == 4 || k == 5 ? s : 0.0f);
    }
  });
  return best;
}

// Node tests (i) and (ii) of the quantised box (wx, wy, wz) of a tree with dequantisation (q_lo, q_scale) against the query triangle
// with bounds m +- eq, normal nq, kq = dot(nq, m - p0) and normal error eps (all in the walked space).  b: the deflated squared gap of
// test (i).  True: the box is open.  Comparisons are written so that a NaN opens the box.
__device__ __forceinline__ bool triangle_box(uint32_t wx, uint32_t wy, uint32_t wz, F3 m, F3 eq, F3 nq, float kq, float eps, F3 q_lo, F3 q_scale, float slack,
                                             float scale2, float rho, float best, float& b) {
  F3 lo, hi;
  box_planes(wx, wy, wz, q_lo, q_scale, lo, hi);
  const float ex = (hi.x - lo.x) * 0.5f, ey = (hi.y - lo.y) * 0.5f, ez = (hi.z - lo.z) * 0.5f;
  const float mx = m.x - (lo.x + hi.x) * 0.5f, my = m.y - (lo.y + hi.y) * 0.5f, mz = m.z - (lo.z + hi.z) * 0.5f;
  const float gx = fmaxf(((__builtin_fabsf(mx) - ex) - eq.x) - slack, 0.0f);
  const float gy = fmaxf(((__builtin_fabsf(my) - ey) - eq.y) - slack, 0.0f);
  const float gz = fmaxf(((__builtin_fabsf(mz) - ez) - eq.z) - slack, 0.0f);
  b = (gx * gx + gy * gy + gz * gz) * scale2;
  bool open = !(b > best);   // (inclusive, and an unbounded best opens all)
#if RT_TRIANGLE_PLANE
  // dot(nq, c - p0) = kq - dot(nq, m - c)
  const float infl = slack + rho;
  const float dist = __builtin_fabsf(kq - ((nq.x * mx + nq.y * my) + nq.z * mz));
  const float reach = ((ex + infl) * __builtin_fabsf(nq.x) + (ey + infl) * __builtin_fabsf(nq.y)) + ((ez + infl) * __builtin_fabsf(nq.z) + eps);
  open = open && !(dist > reach);
#endif
  return open;
}

struct NearestTriangle {
  static constexpr uint32_t STRIDE = 3;
  struct Params { float qu = 0.f, qv = 0.f; };   // the query's point of the nearest pair
  F3 w0 = mk3(0, 0, 0), w1 = w0, w2 = w0;     // the vertices in world space
  F3 m = w0, eq = w0, nq = w0;                // bounds' centre and half extents, and the normal, in the space of the tree being walked
  float kq = 0.f, eps = 0.f;
  float rho = 0.f;                            // the reach of the best d2 in that space's units, rounded up
  __device__ __forceinline__ bool load(const NearestArgs& a, uint32_t pt, float& r_max, float& pmag, int& against) {
    const float4* qp = a.records + 3u * (size_t)pt;
    const float4 r0 = ld_stream(&qp[0]), r1 = ld_stream(&qp[1]), r2 = ld_stream(&qp[2]);
    w0 = mk3(r0.x, r0.y, r0.z); w1 = mk3(r1.x, r1.y, r1.z); w2 = mk3(r2.x, r2.y, r2.z); r_max = r0.w; against = (int)__float_as_uint(r2.w);
    pmag = fmaxf(fmaxf(fmaxf(fmaxf(__builtin_fabsf(r0.x), __builtin_fabsf(r0.y)), __builtin_fabsf(r0.z)),
                       fmaxf(fmaxf(__builtin_fabsf(r1.x), __builtin_fabsf(r1.y)), __builtin_fabsf(r1.z))),
                 fmaxf(fmaxf(__builtin_fabsf(r2.x), __builtin_fabsf(r2.y)), __builtin_fabsf(r2.z)));
    return finite_bits(r0.x) && finite_bits(r0.y) && finite_bits(r0.z) && finite_bits(r1.x) && finite_bits(r1.y) && finite_bits(r1.z) &&
           finite_bits(r2.x) && finite_bits(r2.y) && finite_bits(r2.z) && r0.w >= 0.0f;
  }
  // the triangle p0 p1 p2 of the walked space as bounds and plane
  __device__ __forceinline__ void hold(F3 p0, F3 p1, F3 p2) {
    const F3 lo = mk3(fminf(fminf(p0.x, p1.x), p2.x), fminf(fminf(p0.y, p1.y), p2.y), fminf(fminf(p0.z, p1.z), p2.z));
    const F3 hi = mk3(fmaxf(fmaxf(p0.x, p1.x), p2.x), fmaxf(fmaxf(p0.y, p1.y), p2.y), fmaxf(fmaxf(p0.z, p1.z), p2.z));
    m = mk3(lo.x * 0.5f + hi.x * 0.5f, lo.y * 0.5f + hi.y * 0.5f, lo.z * 0.5f + hi.z * 0.5f);
    eq = mk3(hi.x * 0.5f - lo.x * 0.5f, hi.y * 0.5f - lo.y * 0.5f, hi.z * 0.5f - lo.z * 0.5f);
#if RT_TRIANGLE_PLANE
    nq = cross3(sub3(p1, p0), sub3(p2, p0));
    kq = dot3(nq, sub3(m, p0));
    const float L = 2.0f * fmaxf(fmaxf(eq.x, eq.y), eq.z);
    eps = 7.62939453125e-06f * (L * L * L);   // 2^-17 L^3
#endif
  }
  __device__ __forceinline__ void to_world() { hold(w0, w1, w2); }
  __device__ __forceinline__ F3 enter(const InstanceDev* I) {
    hold(xform_point(I->w2o, w0), xform_point(I->w2o, w1), xform_point(I->w2o, w2));
    return mk3(fmaxf(fmaxf(__builtin_fabsf(w0.x), __builtin_fabsf(w1.x)), __builtin_fabsf(w2.x)),
               fmaxf(fmaxf(__builtin_fabsf(w0.y), __builtin_fabsf(w1.y)), __builtin_fabsf(w2.y)),
               fmaxf(fmaxf(__builtin_fabsf(w0.z), __builtin_fabsf(w1.z)), __builtin_fabsf(w2.z)));
  }
  __device__ __forceinline__ void reach(float best, float scale2) { rho = __builtin_sqrtf(best / scale2) * SW_T_HI; }
  __device__ __forceinline__ bool open(uint32_t wx, uint32_t wy, uint32_t wz, F3 q_lo, F3 q_scale, float slack, float scale2, float best, float& b) const {
    return triangle_box(wx, wy, wz, m, eq, nq, kq, eps, q_lo, q_scale, slack, scale2, rho, best, b);
  }
  __device__ __forceinline__ float test(F3 a, F3 ab, F3 ac, float& u, float& v, Params& p) const { return triangle_tri(w0, w1, w2, a, ab, ac, u, v, p.qu, p.qv); }
  __device__ __forceinline__ static void store(const NearestArgs& a, uint32_t pt, Params p) {
    if (a.params) { a.params[2u * (size_t)pt] = p.qu; a.params[2u * (size_t)pt + 1u] = p.qv; }
  }
  __device__ __forceinline__ bool own(const NearestArgs& a, uint32_t pt, int ii) const {
    const float4* qp = a.records + 3u * (size_t)pt;
    return (int)__float_as_uint(qp[2].w) < 0 && ii == (int)__float_as_uint(qp[1].w);
  }
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_TRIANGLE_WAVES_PER_EU))) void k_closest_triangle(NearestArgs a) { nearest_body<NearestTriangle, false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_TRIANGLE_WAVES_PER_EU))) void k_closest_triangle_count(NearestArgs a) { nearest_body<NearestTriangle, true>(a); }

// The side of the reported triangle's plane the query's point of the nearest pair lies on, into word 7 of its rt_hit_attr (after
// k_hit_attr): k_closest_side's rule at p = (P0 + qu g0) + qv g2, g0 = P1 - P0, g2 = P2 - P0 (per component), 0 on a miss.
__global__ __launch_bounds__(256) void k_triangle_side(SceneDev sc, const float4* __restrict__ tris, const float* __restrict__ params, const HitRec* __restrict__ hits,
                                                      uint32_t* __restrict__ attr, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const HitRec hr = hits[i];
  uint32_t kind = 0u;
  if (hr.inst >= 0) {
    const float4 r0 = tris[3u * (size_t)i], r1 = tris[3u * (size_t)i + 1u], r2 = tris[3u * (size_t)i + 2u];
    const float qu = params[2u * (size_t)i], qv = params[2u * (size_t)i + 1u];
    const float4 p = make_float4((r0.x + qu * (r1.x - r0.x)) + qv * (r2.x - r0.x), (r0.y + qu * (r1.y - r0.y)) + qv * (r2.y - r0.y),
                                 (r0.z + qu * (r1.z - r0.z)) + qv * (r2.z - r0.z), 0.0f);
    kind = closest_side_word(sc, &p, hr);
  }
  attr[8u * (size_t)i + 7u] = kind;
}

void launch_triangle_side(const SceneDev& sc, const float4* tris, const float* params, const HitRec* hits, float4* attr, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_triangle_side, dim3((n + 255u) / 256u), dim3(256), 0, s, sc, tris, params, hits, reinterpret_cast<uint32_t*>(attr), n);
}
