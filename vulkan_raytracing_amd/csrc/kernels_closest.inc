// kernels_closest.inc — included by kernels.hip after walk_nearest.inc (product and alt translation units alike).
// rt_closest_point_device: for every query point the nearest point of the scene's surface within the record's radius.  The point shape
// of the nearest-pair family (walk_nearest.inc: the walk, the deflation, the key), one lane per point:
//
//  * the record is 16 bytes, (p.xyz, r_max); the point is held in the space of the tree being walked: in world space for TLAS nodes,
//    in the instance's object space for BLAS nodes;
//  * the node test is the deflated point-to-box distance on the dequantised planes (box_bound);
//  * the triangle test is the canonical sequence of DESIGN.md §5 in world space (closest_tri).
#ifndef RT_CLOSEST_WAVES_PER_EU
#define RT_CLOSEST_WAVES_PER_EU 4   /* the record-level walks' budget */
#endif

// s_i of every instance: a lower bound on the smallest singular value of the linear part L of o2w, tight (to 1e-6) for every matrix.
// G = L^T L in binary64, four cyclic Jacobi sweeps, then Gershgorin on what is left: lambda_min >= min_k (G_kk - sum_j |G_kj|).
// out[1 + i] = s_i.  out[0] (zero before the launch) becomes the largest row-term magnitude max_r (|o2w_r| . |mesh bounds| + |o2w_r3|)
// over the instances: the scale of the rounding of a = xform_point(o2w, v0), which exceeds the world coordinates when a translation
// cancels the mesh's own offset; the walk's world-space slack takes it in, so TLAS nodes are not pruned below that error either.
__global__ __launch_bounds__(256) void k_closest_scale(const InstanceDev* __restrict__ inst, float* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float* m = inst[i].o2w;
  if (((inst[i].mask >> INST_WORLD_MASK_SHIFT) & 0xFFu) != 0u) {   // (an empty mesh and a void record have mask 0 and no bounds)
    const float* ql = inst[i].q_lo; const float* qs = inst[i].q_scale;
    float bm[3], mw = 0.f;
    for (int k = 0; k < 3; k++) bm[k] = fmaxf(__builtin_fabsf(ql[k]), __builtin_fabsf(__builtin_fmaf(65535.0f, qs[k], ql[k])));
    for (int r = 0; r < 3; r++)
      mw = fmaxf(mw, __builtin_fabsf(m[4 * r]) * bm[0] + __builtin_fabsf(m[4 * r + 1]) * bm[1] + __builtin_fabsf(m[4 * r + 2]) * bm[2] + __builtin_fabsf(m[4 * r + 3]));
    if (!(mw <= 3.0e38f)) mw = __builtin_inff();   // (NaN too: an infinite slack, nothing is pruned)
    atomicMax(reinterpret_cast<uint32_t*>(out), __float_as_uint(mw));   // (non-negative floats order as their bits)
  }
  double g00 = 0, g01 = 0, g02 = 0, g11 = 0, g12 = 0, g22 = 0;
  for (int r = 0; r < 3; r++) {
    const double x = m[4 * r], y = m[4 * r + 1], z = m[4 * r + 2];
    g00 += x * x; g01 += x * y; g02 += x * z; g11 += y * y; g12 += y * z; g22 += z * z;
  }
  const double tr = g00 + g11 + g22;
  // one Jacobi rotation in the plane (p, q) of the symmetric matrix (app, aqq, apq); apr / aqr are the couplings to the third axis
  auto rotate = [](double& app, double& aqq, double& apq, double& apr, double& aqr) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
    const double c = 1.0 / __builtin_sqrt(t * t + 1.0), s = t * c;
    app -= t * apq; aqq += t * apq; apq = 0.0;
    const double pr = c * apr - s * aqr, qr = s * apr + c * aqr;
    apr = pr; aqr = qr;
  };
  for (int sweep = 0; sweep < 4; sweep++) {
    rotate(g00, g11, g01, g02, g12);
    rotate(g00, g22, g02, g01, g12);
    rotate(g11, g22, g12, g01, g02);
  }
  const double a01 = __builtin_fabs(g01), a02 = __builtin_fabs(g02), a12 = __builtin_fabs(g12);
  double lam = __builtin_fmin(__builtin_fmin(g00 - a01 - a02, g11 - a01 - a12), g22 - a02 - a12);
  lam = lam * (1.0 - 1e-6) - 1e-9 * tr;   // the roundings of the sweeps (binary64, a few 1e-16 tr) and of the conversion below
  float s = 0.0f;
  if (lam > 0.0 && tr < 1e60) { s = (float)__builtin_sqrt(lam); s *= 0.99999988f; }
  out[1u + i] = s;   // (NaN / inf transforms: 0 — the instance's boxes do not prune)
}

// The canonical point-to-triangle distance (DESIGN.md §5): Ericson, Real-Time Collision Detection §5.1.5, in binary32 and in world
// space.  a, ab, ac: the packet through the instance's o2w.  Returns d2 (NaN for some zero-area triangles) and (u, v) of B and C.
__device__ __forceinline__ float closest_tri(F3 p, F3 a, F3 ab, F3 ac, float& u, float& v) {
  const F3 ap = sub3(p, a);
  const float d1 = dot3(ab, ap), d2 = dot3(ac, ap);
  const F3 bp = sub3(ap, ab);
  const float d3 = dot3(ab, bp), d4 = dot3(ac, bp);
  const F3 cp = sub3(ap, ac);
  const float d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  if (d1 <= 0.0f && d2 <= 0.0f) { u = 0.0f; v = 0.0f; }                                   // vertex A
  else if (d3 >= 0.0f && d4 <= d3) { u = 1.0f; v = 0.0f; }                                // vertex B
  else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { u = d1 / (d1 - d3); v = 0.0f; }      // edge AB
  else if (d6 >= 0.0f && d5 <= d6) { u = 0.0f; v = 1.0f; }                                // vertex C
  else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { u = 0.0f; v = d2 / (d2 - d6); }      // edge AC
  else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {                        // edge BC
    v = (d4 - d3) / ((d4 - d3) + (d5 - d6)); u = 1.0f - v;
  } else {                                                                                // face
    const float denom = 1.0f / ((va + vb) + vc);
    u = vb * denom; v = vc * denom;
  }
  const F3 c = mk3(ap.x - (u * ab.x + v * ac.x), ap.y - (u * ab.y + v * ac.y), ap.z - (u * ab.z + v * ac.z));
  return dot3(c, c);
}

// the deflated squared distance from q to the quantised box (wx, wy, wz) of a tree with dequantisation (q_lo, q_scale): every axis
// distance shortened by `slack`, the sum times `scale2`
__device__ __forceinline__ float box_bound(uint32_t wx, uint32_t wy, uint32_t wz, F3 q, F3 q_lo, F3 q_scale, float slack, float scale2) {
  F3 lo, hi;
  box_planes(wx, wy, wz, q_lo, q_scale, lo, hi);
  const float dx = fmaxf(fmaxf(lo.x - q.x, q.x - hi.x) - slack, 0.0f);
  const float dy = fmaxf(fmaxf(lo.y - q.y, q.y - hi.y) - slack, 0.0f);
  const float dz = fmaxf(fmaxf(lo.z - q.z, q.z - hi.z) - slack, 0.0f);
  return (dx * dx + dy * dy + dz * dz) * scale2;
}

struct NearestPoint {
  static constexpr uint32_t STRIDE = 1;
  struct Params {};
  F3 wp = mk3(0, 0, 0), q = wp;               // the point in world space; in the space of the tree being walked
  __device__ __forceinline__ bool load(const NearestArgs& a, uint32_t pt, float& r_max, float& pmag, int& against) {
    const float4 r = ld_stream(&a.records[pt]);
    wp = mk3(r.x, r.y, r.z); r_max = r.w; against = -1;
    pmag = fmaxf(fmaxf(__builtin_fabsf(r.x), __builtin_fabsf(r.y)), __builtin_fabsf(r.z));
    return finite_bits(r.x) && finite_bits(r.y) && finite_bits(r.z) && r.w >= 0.0f;
  }
  __device__ __forceinline__ void to_world() { q = wp; }
  __device__ __forceinline__ F3 enter(const InstanceDev* I) { q = xform_point(I->w2o, wp); return wp; }
  __device__ __forceinline__ void reach(float, float) {}   // (the point's node test has no use for it)
  __device__ __forceinline__ bool open(uint32_t wx, uint32_t wy, uint32_t wz, F3 q_lo, F3 q_scale, float slack, float scale2, float best, float& b) const {
    b = box_bound(wx, wy, wz, q, q_lo, q_scale, slack, scale2);
    return !(b > best);   // (inclusive, and an unbounded best opens all)
  }
  __device__ __forceinline__ float test(F3 a, F3 ab, F3 ac, float& u, float& v, Params&) const { return closest_tri(wp, a, ab, ac, u, v); }
  __device__ __forceinline__ static void store(const NearestArgs&, uint32_t, Params) {}
};

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_CLOSEST_WAVES_PER_EU))) void k_closest_point(NearestArgs a) { nearest_body<NearestPoint, false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_CLOSEST_WAVES_PER_EU))) void k_closest_point_count(NearestArgs a) { nearest_body<NearestPoint, true>(a); }

// The side of the reported triangle's plane the query point lies on, into word 7 of its rt_hit_attr (after k_hit_attr): front when
// s = dot(cross(e1, e2), xform_point(w2o, p) - v0) < 0, e1 / e2 / v0 from the vertex buffer as k_hit_kind forms them, inverted by
// FLIP_FACING; 0 on a miss.  The kind k_hit_kind reports for a ray from the point that hits that triangle.
__device__ __forceinline__ uint32_t closest_side_word(const SceneDev& sc, const float4* __restrict__ point, const HitRec h) {
  if (h.inst < 0) return 0u;
  const InstanceDev* I = sc.inst + h.inst;
  const float4 r = *point;
  const F3 po = xform_point(I->w2o, mk3(r.x, r.y, r.z));
  const uint32_t* ix = sc.idx + I->first_index + 3u * (uint32_t)h.prim;
  const float* vb = sc.verts + I->first_float;
  const float* p0 = vb + 6u * ix[0]; const float* p1 = vb + 6u * ix[1]; const float* p2 = vb + 6u * ix[2];
  const F3 e1 = mk3(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]), e2 = mk3(p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]);
  const float s = dot3(cross3(e1, e2), mk3(po.x - p0[0], po.y - p0[1], po.z - p0[2]));
  const bool front = ((s < 0.0f) == FRONT_IS_DET_NEGATIVE) != (((I->mask >> 8) & INST_FLAG_FLIP_FACING) != 0u);
  return front ? 0xFEu : 0xFFu;
}
__global__ __launch_bounds__(256) void k_closest_side(SceneDev sc, const float4* __restrict__ points, const HitRec* __restrict__ hits, uint32_t* __restrict__ attr,
                                                     uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  attr[8u * (size_t)i + 7u] = closest_side_word(sc, points + i, hits[i]);
}

void launch_closest_scale(const SceneDev& sc, float* inst_scale, hipStream_t s) {
  hipMemsetAsync(inst_scale, 0, sizeof(float), s);
  if (sc.n_inst > 0) hipLaunchKernelGGL(k_closest_scale, dim3(((uint32_t)sc.n_inst + 255u) / 256u), dim3(256), 0, s, sc.inst, inst_scale, (uint32_t)sc.n_inst);
}

void launch_closest_side(const SceneDev& sc, const float4* points, const HitRec* hits, float4* attr, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_closest_side, dim3((n + 255u) / 256u), dim3(256), 0, s, sc, points, hits, reinterpret_cast<uint32_t*>(attr), n);
}
