// kernels_sweep.inc — included by kernels.hip after kernels_overlap.inc (product and alt translation units alike).
// rt_sweep_spheres_device: for every sweep record (o, r, d, tmax) the first triangle of the scene that the sphere of radius r touches while
// its centre moves along p(t) = o + t d, t in [0, tmax].  A record-level walk of its own (walk_common.inc: the stack, the chunk feed,
// the trip exit, the counters), one lane per sweep: no frame kernel and no existing query kernel changes.
//
//  * the node test is the slab test of the centre's path against the dequantised child boxes inflated by the radius (DESIGN.md §5
//    "Sphere sweeps"): by R(E) = sqrt(r^2 + 2^-16 L^2) (1 + 2^-13) + 2^-10 L with L = r + 2 E, E the box's own diagonal in world units (no
//    triangle under the box has a longer edge; L bounds the feature offsets whose squares the canonical quadratics cancel), plus 2^-16
//    of the magnitudes that enter the canonical contact (the origin, the TLAS bounds, the row terms of every o2w: word 0 of
//    k_closest_scale's array).  Inside instance i the path goes through w2o as in k_trace, E is the object diagonal times the Frobenius
//    norm of o2w's linear part, and the inflation is R(E) / s_i (s_i <= sigma_min(o2w), k_closest_scale) plus 2^-16 of the object-space
//    magnitudes.  The entry time is shortened and the exit time lengthened by 2^-13 of themselves.  s_i == 0 or a non-finite bound: an
//    infinite inflation, the instance's boxes do not prune.  Comparisons are written so that a node with NaN times only is opened;
//  * the nearer child first, the other pushed; a child is skipped only when its entry time EXCEEDS the best t (ties still arrive);
//  * the triangle test is the canonical sequence of DESIGN.md §5 in world space (sweep_tri): it depends on the sweep record, the instance
//    record and the packet only, so the result is the minimum of the key (t, inst, prim) whatever the tree.
#ifndef RT_SWEEP_WAVES_PER_EU
#define RT_SWEEP_WAVES_PER_EU 4   /* the record-level walks' budget */
#endif

struct SweepArgs {
  SceneDev sc;
  const float4* sweeps;        // n records of 32 bytes: (o.xyz, r), (d.xyz, tmax)
  const float* inst_scale;     // k_closest_scale: [0] the largest row-term magnitude of any instance's o2w, [1 + i] s_i
  uint32_t cull_mask;
  uint32_t n;
  HitRec* hits;                // n records
  uint32_t* cursor;            // chunk cursor (zero before the launch)
  uint32_t* counters;          // the query's counter block (counting form: CNT_NODE_VISITS, CNT_TRI_TESTS)
  int32_t* ovf_stack;          // ovf_stride ints per thread of the grid
};

constexpr float SW_QUAD = 1.52587890625e-05f;      // 2^-16: the share of L^2 the canonical quadratics may lose in the squared distance
constexpr float SW_FACE = 9.5367431640625e-07f;     // 2^-20: (2^-10)^2, the face contact's residual against the longer edge, squared
constexpr float SW_T_LO = 0.9998779296875f;        // 1 - 2^-13: factor on a box's entry time
constexpr float SW_T_HI = 1.0001220703125f;        // 1 + 2^-13: factor on a box's exit time and on the inflation

// one candidate root t = tc + tp of a feature with the contact's barycentrics (uu, vv): it replaces (t, u, v) when it lies in
// [0, tmax] and precedes t (strictly: the earlier feature keeps a tie; a NaN fails every comparison)
__device__ __forceinline__ void sweep_take(float tc, float tp, float tmax, float uu, float vv, bool ok, float& t, float& u, float& v) {
  const float tt = tc + tp;
  if (ok && tt >= 0.0f && tt <= tmax && tt < t) { t = tt; u = uu; v = vv; }
}

// the entering root of the cylinder of radius r about the line through m's origin with direction e (Ericson §5.3.7's coefficients), m the
// centre relative to that origin at tp = 0: ok when a > 0, disc >= 0 and the segment parameter s lies in [0, 1]
__device__ __forceinline__ bool sweep_edge(F3 m, F3 e, F3 d, float dd, float rr, float& tp, float& s) {
  const float ee = dot3(e, e), me = dot3(m, e), de = dot3(d, e), md = dot3(m, d), mm = dot3(m, m);
  const float a = ee * dd - de * de, b = ee * md - de * me, c = ee * (mm - rr) - me * me;
  const float disc = b * b - a * c;
  tp = (-b - __builtin_sqrtf(disc)) / a;
  s = (me + tp * de) / ee;
  return a > 0.0f && disc >= 0.0f && s >= 0.0f && s <= 1.0f;
}

// the entering root of the sphere of radius r about m's origin: ok when dd > 0 and disc >= 0
__device__ __forceinline__ bool sweep_vertex(F3 m, F3 d, float dd, float rr, float& tp) {
  const float b = dot3(m, d), c = dot3(m, m) - rr;
  const float disc = b * b - dd * c;
  tp = (-b - __builtin_sqrtf(disc)) / dd;
  return dd > 0.0f && disc >= 0.0f;
}

// The canonical first contact of the sphere (o, r) moving along d with the triangle (A, ab, ac), the packet through the instance's o2w
// (DESIGN.md §5 "Sphere sweeps"): binary32, world space.  True: a contact at t in [0, tmax] with the contact point's barycentrics.
__device__ __forceinline__ bool sweep_tri(F3 o, float r, F3 d, float tmax, F3 A, F3 ab, F3 ac, float& t, float& u, float& v) {
  const bool finite = finite_bits(A.x) && finite_bits(A.y) && finite_bits(A.z) && finite_bits(ab.x) && finite_bits(ab.y) && finite_bits(ab.z) &&
                      finite_bits(ac.x) && finite_bits(ac.y) && finite_bits(ac.z);
  if (!finite) return false;
  const float rr = r * r, dd = dot3(d, d);
  // ---- initial overlap: the closest-point sequence for p = o
  const float d2 = closest_tri(o, A, ab, ac, u, v);
  if (d2 <= rr) { t = 0.0f; return true; }
  // ---- re-centre at the path's point nearest to A
  float tc = dot3(sub3(A, o), d) / dd;
  if (!(tc >= 0.0f)) tc = 0.0f;
  if (tc > tmax) tc = tmax;
  const F3 oc = mk3(o.x + tc * d.x, o.y + tc * d.y, o.z + tc * d.z);
  const F3 mp = sub3(oc, A);
  // ---- face
  F3 n = cross3(ab, ac);
  const float nn = dot3(n, n);
  float nd = dot3(n, d);
  if (nd > 0.0f) { n = neg3(n); nd = -nd; }
  if (nn > 0.0f && nd < 0.0f) {
    const float sn = __builtin_sqrtf(nn);
    const float tp = (r * sn - dot3(n, mp)) / nd;
    const float k = r / sn;
    const F3 q = mk3((mp.x + tp * d.x) - k * n.x, (mp.y + tp * d.y) - k * n.y, (mp.z + tp * d.z) - k * n.z);
    const float d00 = dot3(ab, ab), d01 = dot3(ab, ac), d11 = dot3(ac, ac), d20 = dot3(q, ab), d21 = dot3(q, ac);
    const float den = d00 * d11 - d01 * d01;
    const float bv = (d11 * d20 - d01 * d21) / den, bw = (d00 * d21 - d01 * d20) / den;
    // the point those barycentrics stand for must be the contact point: within 2^-10 of the longer edge (SW_FACE is its square)
    const F3 c = mk3(q.x - (bv * ab.x + bw * ac.x), q.y - (bv * ab.y + bw * ac.y), q.z - (bv * ab.z + bw * ac.z));
    const float tt = tc + tp;
    if (bv >= 0.0f && bw >= 0.0f && bv + bw <= 1.0f && dot3(c, c) <= SW_FACE * fmaxf(d00, d11) && tt >= 0.0f && tt <= tmax) { t = tt; u = bv; v = bw; return true; }
  }
  // ---- edges AB, AC, BC, then vertices A, B, C: the smallest accepted root, the earlier feature on a tie
  t = __builtin_inff();
  float tp, s;
  bool ok = sweep_edge(mp, ab, d, dd, rr, tp, s);
  sweep_take(tc, tp, tmax, s, 0.0f, ok, t, u, v);
  ok = sweep_edge(mp, ac, d, dd, rr, tp, s);
  sweep_take(tc, tp, tmax, 0.0f, s, ok, t, u, v);
  const F3 mb = sub3(mp, ab), mc = sub3(mp, ac);
  ok = sweep_edge(mb, sub3(ac, ab), d, dd, rr, tp, s);
  sweep_take(tc, tp, tmax, 1.0f - s, s, ok, t, u, v);
  ok = sweep_vertex(mp, d, dd, rr, tp);
  sweep_take(tc, tp, tmax, 0.0f, 0.0f, ok, t, u, v);
  ok = sweep_vertex(mb, d, dd, rr, tp);
  sweep_take(tc, tp, tmax, 1.0f, 0.0f, ok, t, u, v);
  ok = sweep_vertex(mc, d, dd, rr, tp);
  sweep_take(tc, tp, tmax, 0.0f, 1.0f, ok, t, u, v);
  return t < __builtin_inff();   // (an accepted root precedes the initial +inf, tmax = +inf included)
}

// the inflation of a box whose triangles have no edge longer than E: the radius, what the canonical quadratics may lose of it over
// feature offsets up to L = r + 2 E, and twice the face contact's residual bound
__device__ __forceinline__ float sweep_reach(float wr, float rr, float E) {
  const float L = wr + 2.0f * E;
  return __builtin_sqrtf(rr + SW_QUAD * (L * L)) * SW_T_HI + 9.765625e-04f * L;   // (2^-10 L)
}

// the entry time of the path (q + t / qi per axis) into the quantised box (wx, wy, wz) of a tree with dequantisation (q_lo, q_scale),
// inflated on every side, and whether the path is inside it somewhere in [0, best]: the entry shortened by SW_T_LO, the exit
// lengthened by SW_T_HI.  The inflation is add + sweep_reach(esc * (the box's diagonal)) * inv_s: no triangle under the box has an
// edge longer than the diagonal, esc takes it to world units and inv_s the reach back to the tree's units.  fminf / fmaxf pass a NaN
// over and the comparisons are negated, so a box whose times are all NaN is open.  (A zero direction component with q exactly on an
// inflated plane gives 0 * inf = NaN beside +inf: t_near = +inf, the box is closed.  The plane is the inflated one; the slack keeps
// every canonical contact strictly inside it.)
__device__ __forceinline__ bool sweep_box(uint32_t wx, uint32_t wy, uint32_t wz, F3 q, F3 qi, F3 q_lo, F3 q_scale, float wr, float rr, float add, float inv_s,
                                          float esc, float best, float& t_near) {
  const float ex = (float)((int)(wx >> 16) - (int)(wx & 0xFFFFu)) * q_scale.x, ey = (float)((int)(wy >> 16) - (int)(wy & 0xFFFFu)) * q_scale.y,
              ez = (float)((int)(wz >> 16) - (int)(wz & 0xFFFFu)) * q_scale.z;
  const float diag = __builtin_sqrtf(ex * ex + ey * ey + ez * ez) * SW_T_HI;
  const float infl = add + sweep_reach(wr, rr, esc * diag) * inv_s;
  F3 lo, hi;
  box_planes(wx, wy, wz, q_lo, q_scale, lo, hi);
  const float lx = lo.x - infl, hx = hi.x + infl, ly = lo.y - infl, hy = hi.y + infl, lz = lo.z - infl, hz = hi.z + infl;
  const float ax = (lx - q.x) * qi.x, bx = (hx - q.x) * qi.x;
  const float ay = (ly - q.y) * qi.y, by = (hy - q.y) * qi.y;
  const float az = (lz - q.z) * qi.z, bz = (hz - q.z) * qi.z;
  const float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz));
  const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz));
  t_near = fmaxf(tn * (tn > 0.0f ? SW_T_LO : SW_T_HI), 0.0f);
  const float t_far = tf * (tf > 0.0f ? SW_T_HI : SW_T_LO);
  return !(t_near > t_far) && !(t_near > best);
}

template <bool COUNT>
__device__ __forceinline__ void sweep_body(const SweepArgs& a) {
  __shared__ int s_stack[4][STACK2_LDS][64];
  WalkStack st(s_stack, a.ovf_stack, a.sc.ovf_stride);
  WalkFeed feed;
  constexpr int NONE = 0x7FFFFFFF;            // best_inst / best_prim before the first candidate: every (inst, prim) precedes it

  bool need = true;
  uint32_t pt = 0;
  F3 wo = mk3(0, 0, 0), wd = wo;              // the sweep in world space
  float wr = 0.f, tmax = 0.f;
  F3 q = wo, qi = wo;                         // origin and reciprocal direction in the space of the tree being walked
  float w_slack = 0.f, add = 0.f, inv_s = 1.f, esc = 1.f;   // the inflation's parts in the space of that tree (sweep_box)
  F3 q_lo = wo, q_scale = wo;                 // dequantisation of that tree
  float best = 0.f, best_u = 0.f, best_v = 0.f;
  int best_prim = NONE, best_inst = NONE;
  int cur = REF_DONE, cur_inst = -1;
  unsigned long long cnt_nodes = 0, cnt_tris = 0;

  auto world_space = [&]() {
    q = wo; qi = mk3(1.0f / wd.x, 1.0f / wd.y, 1.0f / wd.z); add = w_slack; inv_s = 1.0f; esc = 1.0f;
    tlas_dequant(a.sc, q_lo, q_scale);
  };

  for (;;) {
    // ---- refill: idle lanes take the next records of the wave's chunk
    const uint32_t rec = feed.take(__ballot(need), a.cursor, a.n);
    if (need && rec != WALK_NONE) {
      pt = rec;
      const float4 r0 = ld_stream(&a.sweeps[2u * (size_t)pt]), r1 = ld_stream(&a.sweeps[2u * (size_t)pt + 1u]);
      wo = mk3(r0.x, r0.y, r0.z); wr = r0.w; wd = mk3(r1.x, r1.y, r1.z); tmax = r1.w;
      const bool valid = finite_bits(r0.x) && finite_bits(r0.y) && finite_bits(r0.z) && finite_bits(r0.w) && r0.w >= 0.0f && finite_bits(r1.x) &&
                         finite_bits(r1.y) && finite_bits(r1.z) && (r1.x != 0.0f || r1.y != 0.0f || r1.z != 0.0f) && r1.w >= 0.0f;
      best = tmax; best_u = 0.f; best_v = 0.f; best_prim = NONE; best_inst = NONE;
      const float mag = fmaxf(fmaxf(__builtin_fabsf(r0.x), __builtin_fabsf(r0.y)), __builtin_fabsf(r0.z));
      w_slack = CP_ABS * fmaxf(tlas_magnitude(a.sc, mag), a.inst_scale[0]);
      world_space();
      cur_inst = -1;
      st.reset(); cur = valid ? a.sc.tlas_root : REF_DONE;
      need = false;
    }
    if (__ballot(!need) == 0) break;   // every lane idle and the records used up

    // ---- interior nodes: every lane at one takes a visit; the trip repeats while most live lanes are interior
    for (;;) {
      if (cur >= 0) {
        uint4 Q0, Q1;
        walk_node(a.sc, cur, Q0, Q1);
        if (COUNT) cnt_nodes++;
        float n0, n1;
        const bool h0 = sweep_box(Q0.x, Q0.y, Q0.z, q, qi, q_lo, q_scale, wr, wr * wr, add, inv_s, esc, best, n0) && box_present(Q0.x);
        const bool h1 = sweep_box(Q0.w, Q1.x, Q1.y, q, qi, q_lo, q_scale, wr, wr * wr, add, inv_s, esc, best, n1) && box_present(Q0.w);
        if (h0 && h1) {
          const bool swap = n1 < n0;
          st.push(swap ? (int)Q1.z : (int)Q1.w);
          cur = swap ? (int)Q1.w : (int)Q1.z;
        } else if (h0) cur = (int)Q1.z;
        else if (h1) cur = (int)Q1.w;
        else cur = st.pop();
      }
      if (walk_trip_done(need, cur)) break;
    }

    if (!need && cur < 0 && cur > REF_MARK && cur_inst >= 0) {
      // ---- BLAS leaf: the canonical test of every packet, in world space; the smallest key (t, inst, prim) stays
      uint32_t first, nt;
      walk_leaf(cur, first, nt);
      const float* m = a.sc.inst[cur_inst].o2w;
      for (uint32_t j = 0; j < nt; j++) {
        const float4* tp = a.sc.tris + (size_t)(first + j) * 3;
        const float4 T0 = tp[0], T1 = tp[1], T2 = tp[2];
        if (COUNT) cnt_tris++;
        float tt, uu, vv;
        const bool hit = sweep_tri(wo, wr, wd, tmax, xform_point(m, mk3(T0.x, T0.y, T0.z)), xform_vec(m, mk3(T0.w, T1.x, T1.y)),
                                   xform_vec(m, mk3(T1.z, T1.w, T2.x)), tt, uu, vv);
        const int prim = (int)__float_as_uint(T2.y);
        if (hit && (tt < best || (tt == best && (cur_inst < best_inst || (cur_inst == best_inst && prim < best_prim))))) {
          best = tt; best_u = uu; best_v = vv; best_prim = prim; best_inst = cur_inst;
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
      // ---- TLAS leaf: enter the instance if the call's mask lets it (the path -> object space, the inflation in object units)
      const int ii = ~cur;
      const InstanceDev* I = a.sc.inst + ii;
      if (((I->mask >> INST_WORLD_MASK_SHIFT) & a.cull_mask & 0xFFu) != 0u) {
        const float s = a.inst_scale[1 + ii];
        const float* w = I->w2o; const float* o = I->o2w;
        q = xform_point(w, wo);
        const F3 qd = xform_vec(w, wd);
        qi = mk3(1.0f / qd.x, 1.0f / qd.y, 1.0f / qd.z);
        q_lo = mk3(I->q_lo[0], I->q_lo[1], I->q_lo[2]); q_scale = mk3(I->q_scale[0], I->q_scale[1], I->q_scale[2]);
        // magnitudes: the mesh's planes, the terms of q's rows (they may cancel), the terms of o2w's rows over the mesh's bounds
        const F3 bm = mk3(fmaxf(__builtin_fabsf(q_lo.x), __builtin_fabsf(__builtin_fmaf(65535.0f, q_scale.x, q_lo.x))),
                          fmaxf(__builtin_fabsf(q_lo.y), __builtin_fabsf(__builtin_fmaf(65535.0f, q_scale.y, q_lo.y))),
                          fmaxf(__builtin_fabsf(q_lo.z), __builtin_fabsf(__builtin_fmaf(65535.0f, q_scale.z, q_lo.z))));
        const F3 ap = mk3(__builtin_fabsf(wo.x), __builtin_fabsf(wo.y), __builtin_fabsf(wo.z));
        float om = fmaxf(fmaxf(bm.x, bm.y), bm.z), wm = w_slack;
        for (int r = 0; r < 3; r++) {
          om = fmaxf(om, __builtin_fabsf(w[4 * r]) * ap.x + __builtin_fabsf(w[4 * r + 1]) * ap.y + __builtin_fabsf(w[4 * r + 2]) * ap.z + __builtin_fabsf(w[4 * r + 3]));
          wm = fmaxf(wm, CP_ABS * (__builtin_fabsf(o[4 * r]) * bm.x + __builtin_fabsf(o[4 * r + 1]) * bm.y + __builtin_fabsf(o[4 * r + 2]) * bm.z + __builtin_fabsf(o[4 * r + 3])));
        }
        // an object-space length is at most ||L||_F times itself in world units (L the linear part of o2w); a world reach is at most
        // 1 / s_i times itself in object units (s == 0: an infinite inflation, every box open)
        float fro = 0.f;
        for (int r = 0; r < 3; r++) fro += o[4 * r] * o[4 * r] + o[4 * r + 1] * o[4 * r + 1] + o[4 * r + 2] * o[4 * r + 2];
        esc = __builtin_sqrtf(fro) * SW_T_HI;
        inv_s = 1.0f / s;
        add = CP_ABS * om + wm * inv_s;
        if (!(add <= 3.0e38f)) add = __builtin_inff();
        st.push(REF_MARK);
        cur_inst = ii; cur = I->blas_root;
      } else cur = st.pop();
    }
    if (!need && cur == REF_DONE) {
      // ---- finished: the record, or the miss form with tmax as given
      HitRec h;
      if (best_inst != NONE) { h.t = best; h.u = best_u; h.v = best_v; h.prim = best_prim; h.inst = best_inst; }
      else { h.t = tmax; h.u = 0.f; h.v = 0.f; h.prim = -1; h.inst = -1; }
      a.hits[pt] = h;
      need = true;
    }
  }
  if (COUNT) walk_flush_counters(a.counters, cnt_nodes, cnt_tris);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_SWEEP_WAVES_PER_EU))) void k_sweep_spheres(SweepArgs a) { sweep_body<false>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_SWEEP_WAVES_PER_EU))) void k_sweep_spheres_count(SweepArgs a) { sweep_body<true>(a); }

// The side of the reported triangle's plane the sphere's centre lies on at the contact, into word 7 of its rt_hit_attr (after
// k_hit_attr): k_closest_side's rule at p = o + t d (per component one product and one sum), 0 on a miss.
__global__ __launch_bounds__(256) void k_sweep_side(SceneDev sc, const float4* __restrict__ sweeps, const HitRec* __restrict__ hits, uint32_t* __restrict__ attr,
                                                   uint32_t n) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const HitRec h = hits[i];
  uint32_t kind = 0u;
  if (h.inst >= 0) {
    const InstanceDev* I = sc.inst + h.inst;
    const float4 r0 = sweeps[2u * (size_t)i], r1 = sweeps[2u * (size_t)i + 1u];
    const F3 po = xform_point(I->w2o, mk3(r0.x + h.t * r1.x, r0.y + h.t * r1.y, r0.z + h.t * r1.z));
    const uint32_t* ix = sc.idx + I->first_index + 3u * (uint32_t)h.prim;
    const float* vb = sc.verts + I->first_float;
    const float* p0 = vb + 6u * ix[0]; const float* p1 = vb + 6u * ix[1]; const float* p2 = vb + 6u * ix[2];
    const F3 e1 = mk3(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]), e2 = mk3(p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]);
    const float s = dot3(cross3(e1, e2), mk3(po.x - p0[0], po.y - p0[1], po.z - p0[2]));
    const bool front = ((s < 0.0f) == FRONT_IS_DET_NEGATIVE) != (((I->mask >> 8) & INST_FLAG_FLIP_FACING) != 0u);
    kind = front ? 0xFEu : 0xFFu;
  }
  attr[8u * (size_t)i + 7u] = kind;
}

void launch_sweep_spheres(const SceneDev& sc, const float4* sweeps, uint32_t cull_mask, const float* inst_scale, HitRec* hits, uint32_t n, int32_t* ovf_stack,
                          uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s) {
  SweepArgs a{};
  a.sc = sc; a.sweeps = sweeps; a.inst_scale = inst_scale; a.cull_mask = cull_mask; a.n = n; a.hits = hits; a.counters = counters; a.ovf_stack = ovf_stack;
  launch_walk(k_sweep_spheres, k_sweep_spheres_count, a, counters, counting, cfg, s);
}

void launch_sweep_side(const SceneDev& sc, const float4* sweeps, const HitRec* hits, float4* attr, uint32_t n, hipStream_t s) {
  hipLaunchKernelGGL(k_sweep_side, dim3((n + 255u) / 256u), dim3(256), 0, s, sc, sweeps, hits, reinterpret_cast<uint32_t*>(attr), n);
}
