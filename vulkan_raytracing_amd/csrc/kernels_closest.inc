// kernels_closest.inc — included by kernels.hip (product and alt translation units alike).
// rt_closest_point_device: for every query point the nearest point of the scene's surface within the record's radius.  A record-level
// walk of its own (walk_common.inc: the stack, the chunk feed, the trip exit, the counters), one lane per point: no frame kernel and no
// k_trace instantiation changes.
//
//  * the box test is the point-to-box distance on the dequantised planes: in world space for TLAS nodes, in the instance's object space
//    for BLAS nodes, there times s_i <= sigma_min(linear part of o2w) (k_closest_scale), which makes it a lower bound on the world
//    distance under any affine instance;
//  * the bound is deflated (DESIGN.md §5 "Closest points"): every axis distance by an absolute slack 2^-16 of the magnitudes that enter
//    the canonical d2 (the point, the planes, the rows of the transforms), the sum of squares by 1 - 2^-13, so that it stays below the
//    BINARY32 d2 of every triangle under the box; a subtree is skipped only when its bound EXCEEDS the best d2 (ties still arrive);
//  * the nearer child first, the farther one pushed;
//  * the triangle test is the canonical sequence of DESIGN.md §5 in world space (closest_tri): it depends on the point, the instance
//    record and the packet only, so the result is the minimum of the key (d2, inst, prim) whatever the tree.
#ifndef RT_CLOSEST_WAVES_PER_EU
#define RT_CLOSEST_WAVES_PER_EU 4   /* the record-level walks' budget */
#endif

struct ClosestArgs {
  SceneDev sc;
  const float4* points;        // n records of 16 bytes: (p.xyz, r_max)
  const float* inst_scale;     // k_closest_scale: [0] the largest row-term magnitude of any instance's o2w, [1 + i] s_i
  uint32_t cull_mask;
  uint32_t n;
  HitRec* hits;                // n records
  uint32_t* cursor;            // chunk cursor (zero before the launch)
  uint32_t* counters;          // the query's counter block (counting form: CNT_NODE_VISITS, CNT_TRI_TESTS)
  int32_t* ovf_stack;          // ovf_stride ints per thread of the grid
};

constexpr float CP_ABS = 1.52587890625e-05f;       // 2^-16: absolute slack per unit of magnitude
constexpr float CP_REL = 0.9998779296875f;         // 1 - 2^-13: factor on the squared bound

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

// The entry of instance I (s: its scale of k_closest_scale) by the closest-family point walks (k_closest_point, k_closest_hits): the
// world point wp into object space (q), the dequantisation of the mesh's tree, and the slack of both spaces in object units
// (w_slack: the walk's world-space slack) with the factor on the squared bound.
__device__ __forceinline__ void closest_enter_instance(const InstanceDev* I, float s, F3 wp, float w_slack, F3& q, F3& q_lo, F3& q_scale, float& slack, float& scale2) {
  const float* w = I->w2o; const float* o = I->o2w;
  q = xform_point(w, wp);
  q_lo = mk3(I->q_lo[0], I->q_lo[1], I->q_lo[2]); q_scale = mk3(I->q_scale[0], I->q_scale[1], I->q_scale[2]);
  // magnitudes: the mesh's planes, the terms of q's rows (they may cancel), the terms of o2w's rows over the mesh's bounds
  const F3 bm = mk3(fmaxf(__builtin_fabsf(q_lo.x), __builtin_fabsf(__builtin_fmaf(65535.0f, q_scale.x, q_lo.x))),
                    fmaxf(__builtin_fabsf(q_lo.y), __builtin_fabsf(__builtin_fmaf(65535.0f, q_scale.y, q_lo.y))),
                    fmaxf(__builtin_fabsf(q_lo.z), __builtin_fabsf(__builtin_fmaf(65535.0f, q_scale.z, q_lo.z))));
  const F3 ap = mk3(__builtin_fabsf(wp.x), __builtin_fabsf(wp.y), __builtin_fabsf(wp.z));
  float om = fmaxf(fmaxf(bm.x, bm.y), bm.z), wm = w_slack;
  for (int r = 0; r < 3; r++) {
    om = fmaxf(om, __builtin_fabsf(w[4 * r]) * ap.x + __builtin_fabsf(w[4 * r + 1]) * ap.y + __builtin_fabsf(w[4 * r + 2]) * ap.z + __builtin_fabsf(w[4 * r + 3]));
    wm = fmaxf(wm, CP_ABS * (__builtin_fabsf(o[4 * r]) * bm.x + __builtin_fabsf(o[4 * r + 1]) * bm.y + __builtin_fabsf(o[4 * r + 2]) * bm.z + __builtin_fabsf(o[4 * r + 3])));
  }
  slack = CP_ABS * om + wm / s;   // (s == 0: an infinite slack, every bound 0)
  scale2 = CP_REL * (s * s);
}

template <bool COUNT>
__device__ __forceinline__ void closest_body(const ClosestArgs& a) {
  __shared__ int s_stack[4][STACK2_LDS][64];
  WalkStack st(s_stack, a.ovf_stack, a.sc.ovf_stride);
  WalkFeed feed;
  constexpr int NONE = 0x7FFFFFFF;            // best_inst / best_prim before the first candidate: every (inst, prim) precedes it

  bool need = true;
  uint32_t pt = 0;
  F3 wp = mk3(0, 0, 0), q = wp;               // the point in world space; in the space of the tree being walked
  float w_slack = 0.f, slack = 0.f, scale2 = CP_REL;
  F3 q_lo = wp, q_scale = wp;                 // dequantisation of that tree
  float best = 0.f, best_u = 0.f, best_v = 0.f;
  int best_prim = NONE, best_inst = NONE;
  int cur = REF_DONE, cur_inst = -1;
  unsigned long long cnt_nodes = 0, cnt_tris = 0;

  auto world_space = [&]() { q = wp; slack = w_slack; scale2 = CP_REL; tlas_dequant(a.sc, q_lo, q_scale); };

  for (;;) {
    // ---- refill: idle lanes take the next points of the wave's chunk
    const uint32_t rec = feed.take(__ballot(need), a.cursor, a.n);
    if (need && rec != WALK_NONE) {
      pt = rec;
      const float4 r = ld_stream(&a.points[pt]);
      wp = mk3(r.x, r.y, r.z);
      const bool valid = finite_bits(r.x) && finite_bits(r.y) && finite_bits(r.z) && r.w >= 0.0f;
      best = r.w * r.w; best_u = 0.f; best_v = 0.f; best_prim = NONE; best_inst = NONE;
      const float pmag = fmaxf(fmaxf(__builtin_fabsf(r.x), __builtin_fabsf(r.y)), __builtin_fabsf(r.z));
      w_slack = CP_ABS * fmaxf(fmaxf(pmag, tlas_magnitude(a.sc, 0.f)), a.inst_scale[0]);
      world_space();
      cur_inst = -1;
      st.reset(); cur = valid ? a.sc.tlas_root : REF_DONE;
      need = false;
    }
    if (__ballot(!need) == 0) break;   // every lane idle and the points used up

    // ---- interior nodes: every lane at one takes a visit; the trip repeats while most live lanes are interior
    for (;;) {
      if (cur >= 0) {
        uint4 Q0, Q1;
        walk_node(a.sc, cur, Q0, Q1);
        if (COUNT) cnt_nodes++;
        const float b0 = box_bound(Q0.x, Q0.y, Q0.z, q, q_lo, q_scale, slack, scale2);
        const float b1 = box_bound(Q0.w, Q1.x, Q1.y, q, q_lo, q_scale, slack, scale2);
        // (!(b > best): inclusive, and an unbounded best opens all)
        const bool h0 = box_present(Q0.x) && !(b0 > best);
        const bool h1 = box_present(Q0.w) && !(b1 > best);
        if (h0 && h1) {
          const bool swap = b1 < b0;
          st.push(swap ? (int)Q1.z : (int)Q1.w);
          cur = swap ? (int)Q1.w : (int)Q1.z;
        } else if (h0) cur = (int)Q1.z;
        else if (h1) cur = (int)Q1.w;
        else cur = st.pop();
      }
      if (walk_trip_done(need, cur)) break;
    }

    if (!need && cur < 0 && cur > REF_MARK && cur_inst >= 0) {
      // ---- BLAS leaf: the canonical test of every packet, in world space; the smallest key (d2, inst, prim) stays
      uint32_t first, nt;
      walk_leaf(cur, first, nt);
      const float* m = a.sc.inst[cur_inst].o2w;
      for (uint32_t j = 0; j < nt; j++) {
        const float4* tp = a.sc.tris + (size_t)(first + j) * 3;
        const float4 T0 = tp[0], T1 = tp[1], T2 = tp[2];
        if (COUNT) cnt_tris++;
        float uu, vv;
        const float d2 = closest_tri(wp, xform_point(m, mk3(T0.x, T0.y, T0.z)), xform_vec(m, mk3(T0.w, T1.x, T1.y)), xform_vec(m, mk3(T1.z, T1.w, T2.x)), uu, vv);
        const int prim = (int)__float_as_uint(T2.y);
        if (d2 < best || (d2 == best && (cur_inst < best_inst || (cur_inst == best_inst && prim < best_prim)))) {
          best = d2; best_u = uu; best_v = vv; best_prim = prim; best_inst = cur_inst;
        }
      }
      cur = st.pop();
    }
    if (!need && cur == REF_MARK) {
      // ---- leave the instance
      cur_inst = -1;
      world_space();
      cur = st.pop();
    }
    if (!need && cur < 0 && cur > REF_MARK && cur_inst < 0) {
      // ---- TLAS leaf: enter the instance if the call's mask lets it (point -> object space, the slack of both spaces in object units)
      const int ii = ~cur;
      const InstanceDev* I = a.sc.inst + ii;
      if (((I->mask >> INST_WORLD_MASK_SHIFT) & a.cull_mask & 0xFFu) != 0u) {
        closest_enter_instance(I, a.inst_scale[1 + ii], wp, w_slack, q, q_lo, q_scale, slack, scale2);
        st.push(REF_MARK);
        cur_inst = ii; cur = I->blas_root;
      } else cur = st.pop();
    }
    if (!need && cur == REF_DONE) {
      // ---- finished: the record, or the miss form with the radius as given
      HitRec h;
      if (best_inst != NONE) { h.t = __builtin_sqrtf(best); h.u = best_u; h.v = best_v; h.prim = best_prim; h.inst = best_inst; }
      else { h.t = ld_stream(&a.points[pt]).w; h.u = 0.f; h.v = 0.f; h.prim = -1; h.inst = -1; }
      a.hits[pt] = h;
      need = true;
    }
  }
  if (COUNT) walk_flush_counters(a.counters, cnt_nodes, cnt_tris);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_CLOSEST_WAVES_PER_EU))) void k_closest_point(ClosestArgs a) { closest_body<false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_CLOSEST_WAVES_PER_EU))) void k_closest_point_count(ClosestArgs a) { closest_body<true>(a); }

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

void launch_closest_point(const SceneDev& sc, const float4* points, uint32_t cull_mask, const float* inst_scale, HitRec* hits, uint32_t n, int32_t* ovf_stack,
                          uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s) {
  ClosestArgs a{};
  a.sc = sc; a.points = points; a.inst_scale = inst_scale; a.cull_mask = cull_mask; a.n = n; a.hits = hits; a.counters = counters; a.ovf_stack = ovf_stack;
  launch_walk(k_closest_point, k_closest_point_count, a, counters, counting, cfg, s);
}

void launch_closest_side(const SceneDev& sc, const float4* points, const HitRec* hits, float4* attr, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_closest_side, dim3((n + 255u) / 256u), dim3(256), 0, s, sc, points, hits, reinterpret_cast<uint32_t*>(attr), n);
}
