// kernels_beam.inc — closest-hit traversal of the PRIMARY rays, one walk per PIXEL (round 4; included by kernels.hip behind trace_body and shade_slot).
//
// The (up to four) samples of a pixel leave the same point — the camera — in directions a fraction of a pixel apart
// (src/shader.rgen:62-79), and walk almost the same nodes one after the other in the one-lane-per-ray kernel.  Here one lane walks the
// tree ONCE for all of them: a node's box is tested against the BEAM of the lane's live rays, and only at a leaf is the triangle tested
// against every ray with the canonical test.  Box tests only have to be conservative (DESIGN.md §3), and for rays of one origin the
// conservative test is cheap: on each axis the distance to a plane is P * (1/d_j) with the SAME P = plane - origin for every ray, so
// over the rays it lies between P * min_j(1/d_j) and P * max_j(1/d_j) — two fmas and a min (max) per plane instead of one fma, in the
// quantised form of slab_q: (qs, qb) once for the smallest and once for the largest reciprocal direction of the beam.  On an axis on which
// the rays' directions differ in sign the beam is bounded by the band its rays cannot leave (beam_axis).  The walk is culled by the LARGEST closest-hit distance of the lane's rays.
// What a ray can hit it still hits: its own interval on every axis lies inside the beam's, and the triangle tests are the per-ray
// ones, in the same object-space ray (xform_point / xform_vec of the same world ray) with the same tie rule — hit records bit-identical
// to k_trace's (tests/test_gpu_parity.py test_pixel_beams_are_result_identical).
//
// Queue layout (k_raygen, FrameDev::pixel_runs): bounce queue 0 is a sequence of RUNS of 64 * S slots (S = samples per workgroup of
// k_raygen, <= 4), one per covered tile and sample group, NOT compacted: slot run + 64 j + l is sample j of the tile's pixel l; a
// sample that is not traced (it missed the TLAS, or lies outside the frame) leaves a slot with a zero direction, and gets HIT_DEAD as
// its hit record (k_shade skips it: k_raygen has given it its colour).  A wavefront takes a run; lane l walks pixel l.
// A slot holds a direction and a sample id only: the origin of every primary ray is the camera of its frame and its tile is the run's, so
// k_raygen stores (camera, tile) ONCE per run, in the origin slot of the run's first entry; the wave reads that one address.
// No far-ray logic: the host launches this kernel only in frames without far rays (rt_api far_possible).  With camera records (k_entry)
// a pixel's walk starts at its tile's record, without them at the root of the TLAS.
struct BeamSpace { F3 s0, b0, s1, b1; uint3 rot; };   // (qs, qb) of slab_q for the smallest (0) and the largest (1) reciprocal direction per axis

__device__ __forceinline__ bool slab_beam(uint32_t wx, uint32_t wy, uint32_t wz, const BeamSpace& B, float tmin, float tlim, float& tn) {
  wx = __builtin_amdgcn_alignbit(wx, wx, B.rot.x); wy = __builtin_amdgcn_alignbit(wy, wy, B.rot.y); wz = __builtin_amdgcn_alignbit(wz, wz, B.rot.z);
  const float nx = (float)(wx & 0xFFFFu), fx = (float)(wx >> 16), ny = (float)(wy & 0xFFFFu), fy = (float)(wy >> 16), nz = (float)(wz & 0xFFFFu), fz = (float)(wz >> 16);
  const float x0 = fminf(__builtin_fmaf(nx, B.s0.x, B.b0.x), __builtin_fmaf(nx, B.s1.x, B.b1.x)), x1 = fmaxf(__builtin_fmaf(fx, B.s0.x, B.b0.x), __builtin_fmaf(fx, B.s1.x, B.b1.x));
  const float y0 = fminf(__builtin_fmaf(ny, B.s0.y, B.b0.y), __builtin_fmaf(ny, B.s1.y, B.b1.y)), y1 = fmaxf(__builtin_fmaf(fy, B.s0.y, B.b0.y), __builtin_fmaf(fy, B.s1.y, B.b1.y));
  const float z0 = fminf(__builtin_fmaf(nz, B.s0.z, B.b0.z), __builtin_fmaf(nz, B.s1.z, B.b1.z)), z1 = fmaxf(__builtin_fmaf(fz, B.s0.z, B.b0.z), __builtin_fmaf(fz, B.s1.z, B.b1.z));
  tn = fmaxf(fmaxf(x0, y0), fmaxf(z0, tmin));
  const float tf = fminf(fminf(x1, y1), fminf(z1, tlim));
  return tn <= tf * 1.00002f;
}
// one axis of the beam's ray space: reciprocal directions lo <= hi of the live rays, da = the largest |direction| on this axis, t_far >=
// any distance at which a ray can still be inside the tree's box.  A beam that STRADDLES the axis plane (reciprocals of both signs: the
// pixel's rays run almost parallel to the plane) has no interval in t on this axis — but none of its rays leaves the band
// [o - r, o + r], r = t_far * da, so a box outside the band cannot be hit: in slab_beam's form, with a huge slope K, the "near"
// value K (lo_plane - U) is <= -K for planes up to U - 1 and huge beyond U, the "far" value K (hi_plane - L) likewise (U, L: the band in
// quanta, one quantum of slack each for the rounding).
__device__ __forceinline__ void beam_axis(float lo, float hi, float da, float t_far, float q_lo_minus_o, float q_scale, float& s0, float& b0, float& s1, float& b1, uint32_t& rot) {
  if (lo < 0.0f && hi > 0.0f) {
    const float K = 1.0e30f, inv = 1.0f / q_scale, r = t_far * da;
    const float U = (r - q_lo_minus_o) * inv + 1.0f, L = (-r - q_lo_minus_o) * inv - 1.0f;   // (o + r - q_lo) / q_scale, (o - r - q_lo) / q_scale
    s0 = K; s1 = K; b0 = -K * U; b1 = -K * L; rot = 0u;
  }
  else { s0 = q_scale * lo; b0 = q_lo_minus_o * lo; s1 = q_scale * hi; b1 = q_lo_minus_o * hi; rot = lo < 0.0f ? 16u : 0u; }
}

#define RT_BEAM_EACH(M) M(0) M(1) M(2) M(3)
#ifndef RT_BEAM_KEEP_NUM
#define RT_BEAM_KEEP_NUM RT_KEEP_NUM          /* the interior loop of k_beam goes on while this many eighths of the live lanes are at interior nodes */
#endif
#ifndef RT_BEAM_UNROLL
#define RT_BEAM_UNROLL RT_INTERIOR_UNROLL     /* visits per trip of that loop */
#endif

// k_beam_shade (round 6): the walk that found a pixel's hits shades them.  k_beam ends a run with the hit of every sample in registers and LDS
// (bt0..bt3, s_best), stores them as hit_a / hit_inst for every slot of queue 0, and a second launch (k_shade) reads them back.  Here the
// epilogue of a run hands them to shade_slot (kernels.hip: the one copy of the shading arithmetic) instead: no hit record is written or
// read, and bounce 0 has no k_shade launch.  The host launches it in single frames without counting, tile blobs or shadow runs.
// The argument block carries what the walk and bounce-0 shading read, and nothing else (no BatchTab, one SceneDev): what a kernel does not
// name it does not load, and every word it holds across the interior loop is a scalar register the walk cannot use.
struct BeamShadeUniforms {            // of UniformsDev, under the same names
  float position[3], light_position[3], light_intensity;
  uint32_t max_bounce_count, samples_per_pixel, center_object_type, orbiting_object_type;
};
struct BeamShadeArgs {
  SceneDev sc;
  const float4* ray_o;                // bounce queue 0 (TraceArgs' names: beam_body reads either block)
  const float4* ray_d;
  const uint32_t* tails;
  uint32_t* work;
  uint32_t shard_cap;
  int32_t* ovf_stack;
  uint32_t* counters;
  float tmin;
  const EntryRec* entry;
  float4* next_o;                     // bounce queue 1
  float4* next_d;
  float4* sh_o;                       // the shadow queue, FrameDev's names
  float4* sh_d;
  float4* sh_c;
  uint32_t* sh_e;
  float4* sample_color;
  const EntryRec* light_entry;
  int width, rows, light_tiles, settle_dead_shadow_rays;
  BeamShadeUniforms u;
};
// What shade_slot reads of FrameDev and SceneDev at bounce 0 of such a frame, under the same names; made from the argument block inside the
// kernel, per run.  A pointer is a KargPtr: the PLACE of the pointer in the argument block, read (one scalar load that hits the constant
// cache, ld_const_ptr: a pointer to device memory) where shading uses it — the queue of the next bounce where a mirror pushes a ray, the
// cube map where a sample misses.  Read ahead of the rows, the pointers and uniforms of the epilogue are more words than a wave has
// scalar registers beside the row loop's own, and the rest goes to lanes and comes back inside the loop.
template <typename T> struct KargPtr {
  T* const* at;       // its place in the block, or
  T* held;            // (at == nullptr) the pointer itself, read ahead: what every row uses
  __device__ __forceinline__ operator T*() const { return at != nullptr ? ld_const_ptr(at) : held; }
};
struct BeamShadeFrame {
  KargPtr<float4> ray_o[2], ray_d[2];
  KargPtr<float4> sh_o, sh_d, sh_c; KargPtr<uint32_t> sh_e;
  KargPtr<float4> sample_color;
  KargPtr<uint32_t> counters;
  KargPtr<const EntryRec> light_entry;
  uint32_t shard_cap;
  int width, rows, light_tiles, settle_dead_shadow_rays;
  static constexpr int pixel_runs = 64;       // such a frame has pixel runs (one origin per run: the camera) and no shadow runs
  static constexpr uint32_t sh_base = 0u;
};
struct BeamShadeScene {
  const BeamShadeArgs* ka;
  int n_materials;
  KargPtr<const MaterialDev> materials;
  KargPtr<const uint32_t> prim_material;
  __device__ __forceinline__ operator SceneDev() const {   // for sample_sky, ambient_of, ShadeCarry::fetch: what they do not read of it is not loaded
    SceneDev s = ld_const(&ka->sc);
    s.inst = ld_const_ptr(&ka->sc.inst); s.verts = ld_const_ptr(&ka->sc.verts); s.idx = ld_const_ptr(&ka->sc.idx); s.sky = ld_const_ptr(&ka->sc.sky);
    s.materials = ld_const_ptr(&ka->sc.materials); s.prim_material = ld_const_ptr(&ka->sc.prim_material);
    return s;
  }
};
struct BeamShadeView { const BeamShadeScene& sc; const BeamShadeFrame& f; const BeamShadeUniforms& u; };

template <bool COUNT, bool SHADE = false, typename Args = TraceArgs>
__device__ __forceinline__ void beam_body(const Args& a_entry, const uint32_t run) {
  const Args& a = a_entry;
  __shared__ int s_stack[4][STACK2_LDS + 1][64];
  __shared__ float s_best[4][16][64];    // ray j of lane l: rows 4 j .. 4 j + 3 = u, v, primitive, instance of its closest hit so far (t stays in a register)
  __shared__ float4 s_inst[LDS_INSTANCES ? LDS_INSTANCES : 1][5];
  const int n_lds_inst = a.sc.n_inst < LDS_INSTANCES ? a.sc.n_inst : LDS_INSTANCES;
  if ((int)threadIdx.x < n_lds_inst) {
    const InstanceDev* I = a.sc.inst + threadIdx.x;
    const float4* mp = reinterpret_cast<const float4*>(I->w2o);
    s_inst[threadIdx.x][0] = mp[0]; s_inst[threadIdx.x][1] = mp[1]; s_inst[threadIdx.x][2] = mp[2];
    s_inst[threadIdx.x][3] = make_float4(I->q_lo[0], I->q_lo[1], I->q_lo[2], __int_as_float(I->blas_root));
    s_inst[threadIdx.x][4] = make_float4(I->q_scale[0], I->q_scale[1], I->q_scale[2], __uint_as_float(I->mask));
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  int* const stk = &s_stack[wave][0][lane];
  float* const bst = &s_best[wave][0][lane];                // row r at bst[r * 64]
  const uint32_t S = run >> 6;
  uint64_t cnt_nodes = 0, cnt_tris = 0, diag_iters = 0, diag_busy = 0;   // (counting builds: trips of the interior loop, lanes busy in them)
  const uint64_t diag_t0 = COUNT ? __builtin_readcyclecounter() : 0;
  uint32_t shard = blockIdx.x & (N_SHARDS - 1), tried = 0;

  for (;;) {
    // k_beam_shade: the walk reads its arguments from the block again for every run (scalar loads that hit the constant cache), as the
    // epilogue does.  Held in scalar registers from kernel entry they would be live across the epilogue, which has its own fifty words of
    // pointers and uniforms there: together more than a wave has, and the allocator then spills the walk's into lanes and reads them
    // back inside set_space and the leaf tests.
    Args a_run;
    if constexpr (SHADE) {
      const Args* ka = (const Args*)__builtin_amdgcn_kernarg_segment_ptr();   // (the block is the kernel's first argument: offset 0)
      asm volatile("" : "+s"(ka));
      a_run = ld_const(ka);
      a_run.sc.blas_nodes = ld_const_ptr(&ka->sc.blas_nodes); a_run.sc.tris = ld_const_ptr(&ka->sc.tris); a_run.sc.inst = ld_const_ptr(&ka->sc.inst);
      a_run.ray_o = ld_const_ptr(&ka->ray_o); a_run.ray_d = ld_const_ptr(&ka->ray_d); a_run.tails = ld_const_ptr(&ka->tails); a_run.work = ld_const_ptr(&ka->work);
      a_run.ovf_stack = ld_const_ptr(&ka->ovf_stack); a_run.entry = ld_const_ptr(&ka->entry);
    }
    const Args& a = SHADE ? a_run : a_entry;
    const char* const node_bytes = reinterpret_cast<const char*>(a.sc.blas_nodes);
    // ---- the wave's next run (wave-uniform)
    uint32_t base = 0; bool got = false;
    while (tried < (uint32_t)N_SHARDS) {
      const uint32_t size = ld_cursor(a.tails + shard * CNT_STRIDE);
      uint32_t off = 0;
      if (lane == 0 && size) off = atomicAdd(a.work + shard * CNT_STRIDE, run);
      off = (uint32_t)__builtin_amdgcn_readfirstlane((int)off);
      if (size && off < size) { base = shard * a.shard_cap + off; got = true; break; }
      shard = (shard + 1u) & (N_SHARDS - 1); tried++;
    }
    if (!got) break;
    const uint32_t v0 = base + lane;

    // ---- the lane's pixel: the directions of its live samples (origin and tile are the run's)
    uint32_t alive = 0, sid = 0;   // (sid: of one of the live samples — its frame, in a frame batch)
    F3 co = mk3(0, 0, 0), cd0 = mk3(0, 0, 1), cd1 = cd0, cd2 = cd0, cd3 = cd0;
    float bt0 = -1.0f, bt1 = -1.0f, bt2 = -1.0f, bt3 = -1.0f;   // closest-hit distance so far; a slot without a ray never accepts a hit
    BeamSpace B;
    B.s0 = B.s1 = B.b0 = B.b1 = mk3(0, 0, 0); B.rot = make_uint3(0u, 0u, 0u);
    int cur = REF_DONE, sp = 1, cur_inst = -1;
    uint32_t my_visits = 0;   // (counting builds: node visits of this lane's pixel)

    auto push = [&](int v) {
      if (sp < STACK2_LDS) stk[sp * 64] = v;
      else *reinterpret_cast<volatile int32_t*>(a.ovf_stack + (size_t)(blockIdx.x * 256u + threadIdx.x) * a.sc.ovf_stride + (sp - STACK2_LDS)) = v;   // (the address is made here: deep stacks are rare)
      sp++;
    };
    auto pop = [&]() {
      sp--;
      if (sp < STACK2_LDS) cur = stk[sp * 64];
      else cur = *reinterpret_cast<volatile int32_t*>(a.ovf_stack + (size_t)(blockIdx.x * 256u + threadIdx.x) * a.sc.ovf_stride + (sp - STACK2_LDS));
    };
    // the beam in the space of instance ii (ii < 0: the world, i.e. the TLAS): every live ray exactly as k_trace's to_instance makes it
    // (object-space origin and direction, t preserved), and the (qs, qb) pair of the beam.  The world directions are not kept in
    // registers: they are read from the queue again (a pixel changes its space once or twice in its life).  Returns the instance's root.
    auto set_space = [&](int ii, int& root, uint32_t& imask) {
      const float4 ro = a.ray_o[base];   // the run's one origin word (k_raygen): the camera of its frame — one address for the whole wave
      const F3 wo = mk3(ro.x, ro.y, ro.z);
      F3 w0 = mk3(0, 0, 1), w1 = w0, w2 = w0, w3 = w0;
#define RT_BEAM_LD(j) if (alive & (1u << j)) { const float4 r = a.ray_d[v0 + 64u * j]; w##j = mk3(r.x, r.y, r.z); }
      RT_BEAM_EACH(RT_BEAM_LD)
#undef RT_BEAM_LD
      float qlo3[3] = {a.sc.tlas_q_lo[0], a.sc.tlas_q_lo[1], a.sc.tlas_q_lo[2]}, qsc3[3] = {a.sc.tlas_q_scale[0], a.sc.tlas_q_scale[1], a.sc.tlas_q_scale[2]};
      root = 0; imask = 0xFFu;
      if (ii >= 0) {
        float4 m0, m1, m2, ql, qsc;
        if (ii < n_lds_inst) { m0 = s_inst[ii][0]; m1 = s_inst[ii][1]; m2 = s_inst[ii][2]; ql = s_inst[ii][3]; qsc = s_inst[ii][4]; }
        else {
          const InstanceDev* I = a.sc.inst + ii;
          const float4* mp = reinterpret_cast<const float4*>(I->w2o);
          m0 = mp[0]; m1 = mp[1]; m2 = mp[2];
          ql = make_float4(I->q_lo[0], I->q_lo[1], I->q_lo[2], __int_as_float(I->blas_root));
          qsc = make_float4(I->q_scale[0], I->q_scale[1], I->q_scale[2], __uint_as_float(I->mask));
        }
        root = __float_as_int(ql.w); imask = __float_as_uint(qsc.w);
        if ((imask & 0xFFu) == 0u) return;   // invisible to the ray mask: the space stays what it was
        float m[12];
        m[0] = m0.x; m[1] = m0.y; m[2] = m0.z; m[3] = m0.w; m[4] = m1.x; m[5] = m1.y; m[6] = m1.z; m[7] = m1.w;
        m[8] = m2.x; m[9] = m2.y; m[10] = m2.z; m[11] = m2.w;
        co = xform_point(m, wo);
        cd0 = xform_vec(m, w0); cd1 = xform_vec(m, w1); cd2 = xform_vec(m, w2); cd3 = xform_vec(m, w3);
        qlo3[0] = ql.x; qlo3[1] = ql.y; qlo3[2] = ql.z; qsc3[0] = qsc.x; qsc3[1] = qsc.y; qsc3[2] = qsc.z;
      } else { co = wo; cd0 = w0; cd1 = w1; cd2 = w2; cd3 = w3; }
      float lx = 3.0e38f, ly = 3.0e38f, lz = 3.0e38f, hx = -3.0e38f, hy = -3.0e38f, hz = -3.0e38f, ax = 0.0f, ay = 0.0f, az = 0.0f, l2 = 3.0e38f;
#define RT_BEAM_ID(j) if (alive & (1u << j)) { const float ix = safe_rcp(cd##j.x), iy = safe_rcp(cd##j.y), iz = safe_rcp(cd##j.z); \
        lx = fminf(lx, ix); hx = fmaxf(hx, ix); ly = fminf(ly, iy); hy = fmaxf(hy, iy); lz = fminf(lz, iz); hz = fmaxf(hz, iz); \
        ax = fmaxf(ax, __builtin_fabsf(cd##j.x)); ay = fmaxf(ay, __builtin_fabsf(cd##j.y)); az = fmaxf(az, __builtin_fabsf(cd##j.z)); l2 = fminf(l2, dot3(cd##j, cd##j)); }
      RT_BEAM_EACH(RT_BEAM_ID)
#undef RT_BEAM_ID
      // no ray is inside the tree's box beyond t_far: the farthest corner of the box from the origin over the shortest direction (or the pipeline's tmax)
      const float ex = fmaxf(__builtin_fabsf(qlo3[0] - co.x), __builtin_fabsf(__builtin_fmaf(65535.0f, qsc3[0], qlo3[0]) - co.x));
      const float ey = fmaxf(__builtin_fabsf(qlo3[1] - co.y), __builtin_fabsf(__builtin_fmaf(65535.0f, qsc3[1], qlo3[1]) - co.y));
      const float ez = fmaxf(__builtin_fabsf(qlo3[2] - co.z), __builtin_fabsf(__builtin_fmaf(65535.0f, qsc3[2], qlo3[2]) - co.z));
      const float t_far = fminf(10000.0f, 1.001f * __builtin_sqrtf((ex * ex + ey * ey + ez * ez) / fmaxf(l2, 1.0e-30f)));
      beam_axis(lx, hx, ax, t_far, qlo3[0] - co.x, qsc3[0], B.s0.x, B.b0.x, B.s1.x, B.b1.x, B.rot.x);
      beam_axis(ly, hy, ay, t_far, qlo3[1] - co.y, qsc3[1], B.s0.y, B.b0.y, B.s1.y, B.b1.y, B.rot.y);
      beam_axis(lz, hz, az, t_far, qlo3[2] - co.z, qsc3[2], B.s0.z, B.b0.z, B.s1.z, B.b1.z, B.rot.z);
    };

    {
#define RT_BEAM_ALIVE(j) if (j < S) { const float4 r = ld_stream(&a.ray_d[v0 + 64u * j]); if (r.x != 0.0f || r.y != 0.0f || r.z != 0.0f) { alive |= 1u << j; sid = __float_as_uint(r.w); } }
      RT_BEAM_EACH(RT_BEAM_ALIVE)
#undef RT_BEAM_ALIVE
    }
    if (alive & 1u) bt0 = 10000.0f;   // tmax of src/shader.rgen:87
    if (alive & 2u) bt1 = 10000.0f;
    if (alive & 4u) bt2 = 10000.0f;
    if (alive & 8u) bt3 = 10000.0f;
#pragma unroll
    for (int j = 0; j < 4; j++) { bst[(4 * j + 0) * 64] = 0.0f; bst[(4 * j + 1) * 64] = 0.0f; bst[(4 * j + 2) * 64] = __int_as_float(-1); bst[(4 * j + 3) * 64] = __int_as_float(-1); }
    stk[0] = REF_DONE;
    if (alive != 0u && a.entry == nullptr) {
      // no camera records in this frame: from the root of the TLAS (in a frame batch: of the pixel's frame)
      cur = a.sc.tlas_root + (a.sc.batch_samples ? (int)frame_of(sid, a.sc.batch_samples) * a.sc.tlas_stride : 0);
      int root; uint32_t imask;
      set_space(-1, root, imask);
    } else if (alive != 0u) {
      // the walk starts at the record of the pixel's tile (k_entry), as in k_trace<closest, ENTRY>; the run's first origin slot carries the tile
      const uint32_t tile = __float_as_uint(ld_stream(&a.ray_o[base]).w);
      const int4* rp = reinterpret_cast<const int4*>(a.entry + tile);
      const int4 r0 = rp[0], r1 = rp[1];
      const uint32_t hdr = (uint32_t)r0.x;
      if (hdr != ENTRY_EMPTY) {
        const uint32_t nw = hdr & 15u, ia = hdr >> 8;
        const int wk[6] = {r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) if (k < nw) stk[(1u + k) * 64u] = wk[k];
        sp = 1 + (int)nw;
        cur = r0.y;
        int root; uint32_t imask;
        if (ia != ENTRY_NO_INST) { set_space((int)ia, root, imask); cur_inst = (int)ia; }   // (k_entry never names an invisible instance)
        else set_space(-1, root, imask);
      }
    }

    // ---- the walk: k_trace's phases without the refill (a lane's pixel ends, the wave goes on until its last pixel has)
    typedef __attribute__((address_space(3))) volatile int lds_vint;
    lds_vint* const stk_lds = (lds_vint*)stk;
    for (;;) {
      const uint32_t live = (uint32_t)__builtin_popcountll(__ballot(cur != REF_DONE));
      if (live == 0u) break;
      const uint32_t keep_going = (live * RT_BEAM_KEEP_NUM + 7u) >> 3;
      // (B) interior nodes
      for (;;) {
        const uint32_t n_int = (uint32_t)__builtin_popcountll(__ballot(cur >= 0));
        if (n_int == 0u || n_int < keep_going) break;
        if (COUNT && lane == 0) { diag_iters++; diag_busy += n_int; }
        const float tlim = fmaxf(fmaxf(bt0, bt1), fmaxf(bt2, bt3));
        const bool deep = cur >= 0 && sp + RT_BEAM_UNROLL > STACK2_LDS;
        if (__ballot(deep) == 0ull) {
#pragma unroll
          for (int r = 0; r < RT_BEAM_UNROLL; r++)
            if (cur >= 0) {
              const uint4* np = reinterpret_cast<const uint4*>(node_bytes + ((uint32_t)cur << 5));
              const uint4 Q0 = np[0], Q1 = np[1];
              const int top = stk_lds[(sp - 1) * 64];
              const int2 ch = make_int2((int)Q1.z, (int)Q1.w);
              if (COUNT) { cnt_nodes++; my_visits++; }
              float t0, t1;
              const bool h0 = slab_beam(Q0.x, Q0.y, Q0.z, B, a.tmin, tlim, t0);
              const bool h1 = slab_beam(Q0.w, Q1.x, Q1.y, B, a.tmin, tlim, t1);
              const bool both = h0 && h1, none = !(h0 || h1), swap = t1 < t0;
              const uint32_t pm = 0u - (uint32_t)both;
              stk_lds[(((uint32_t)sp & pm) | ((uint32_t)STACK2_LDS & ~pm)) * 64u] = swap ? ch.x : ch.y;
              const int one = h0 ? ch.x : ch.y;
              cur = both ? (swap ? ch.y : ch.x) : (none ? top : one);
              sp += (both ? 1 : 0) - (none ? 1 : 0);
            }
        } else {
#pragma unroll
          for (int r = 0; r < RT_BEAM_UNROLL; r++)
            if (cur >= 0) {
              const uint4* np = reinterpret_cast<const uint4*>(node_bytes + ((uint32_t)cur << 5));
              const uint4 Q0 = np[0], Q1 = np[1];
              const int2 ch = make_int2((int)Q1.z, (int)Q1.w);
              if (COUNT) { cnt_nodes++; my_visits++; }
              float t0, t1;
              const bool h0 = slab_beam(Q0.x, Q0.y, Q0.z, B, a.tmin, tlim, t0);
              const bool h1 = slab_beam(Q0.w, Q1.x, Q1.y, B, a.tmin, tlim, t1);
              if (h0 && h1) { const bool swap = t1 < t0; push(swap ? ch.x : ch.y); cur = swap ? ch.y : ch.x; }
              else if (h0) cur = ch.x;
              else if (h1) cur = ch.y;
              else pop();
            }
        }
      }
      // (C) BLAS leaf: the canonical test of every live ray on the leaf's packets, k_trace's tie rule
      if (cur < 0 && cur > REF_MARK && cur_inst >= 0) {
        const uint32_t ref = (uint32_t)(~cur);
        const uint32_t first = ref >> 3, count = (ref & 7u) + 1u;
        for (uint32_t k = 0; k < count; k++) {
          const float4* tp = a.sc.tris + (size_t)(first + k) * 3;
          const float4 T0 = tp[0], T1 = tp[1], T2 = tp[2];
          const int prim = (int)__float_as_uint(T2.y);
#define RT_BEAM_TRI(j) if (alive & (1u << j)) { \
            if (COUNT) cnt_tris++; \
            float tt, uu, vv; \
            if (tri_test(T0, T1, T2, co, cd##j, a.tmin, 10000.0f, tt, uu, vv)) { \
              bool better = tt < bt##j; \
              if (tt == bt##j) { const int bi = __float_as_int(bst[(4 * j + 3) * 64]), bp = __float_as_int(bst[(4 * j + 2) * 64]); \
                                 better = bi < 0 || cur_inst < bi || (cur_inst == bi && prim < bp); } \
              if (better) { bt##j = tt; bst[(4 * j + 0) * 64] = uu; bst[(4 * j + 1) * 64] = vv; bst[(4 * j + 2) * 64] = __int_as_float(prim); bst[(4 * j + 3) * 64] = __int_as_float(cur_inst); } \
            } }
          RT_BEAM_EACH(RT_BEAM_TRI)
#undef RT_BEAM_TRI
        }
        pop();
      }
      // leave the instance
      if (cur == REF_MARK) {
        cur_inst = -1;
        pop();
        if (cur >= 0) { int root; uint32_t imask; set_space(-1, root, imask); }
      }
      // TLAS leaf: enter the instance
      if (cur < 0 && cur > REF_MARK && cur_inst < 0) {
        const int ii = ~cur;
        int root; uint32_t imask;
        set_space(ii, root, imask);
        if ((imask & 0xFFu) == 0u) {
          pop();
          if (cur >= 0) set_space(-1, root, imask);
        } else {
          push(REF_MARK);
          cur_inst = ii; cur = root;
        }
      }
    }

    if (COUNT) {
      // how uneven are the pixels of a run?  the longest pixel of the frame, the sum of the runs' longest pixels, the number of runs (rt_stats.tile_diag[0..2])
      uint32_t mx = my_visits;
      for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
      if (lane == 0) {
        atomicMax(a.counters + CNT_TILE_DIAG, mx);
        atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + CNT_TILE_DIAG + 2), (unsigned long long)mx);
        atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + CNT_TILE_DIAG + 4), 1ull);
      }
    }
    if constexpr (SHADE) {
      // ---- the pixel's samples shaded where they lie: sample j of the run's 64 pixels is one convergent call of all 64 lanes
      // (a slot without a ray: HIT_DEAD, as k_beam would have stored it)
      const uint32_t run_shard = (uint32_t)__builtin_amdgcn_readfirstlane((int)shard);
      // What shading reads of the argument block is read HERE, per run, through the kernarg pointer: named as `a.x` the compiler loads every
      // word at kernel entry and carries it across the walk in scalar registers the walk needs (68 of them spilled to lanes of two more
      // VGPRs); the empty asm keeps the loads below it.  A run's scalar loads hit the constant cache.
      // The block is read as what it is, constant memory (ld_const: scalar loads), and the pointers it holds as what they are, pointers to
      // device memory (ld_const_ptr): read as generic ones, every access of the epilogue would be a flat_* instruction.
      const BeamShadeArgs* ka = (const BeamShadeArgs*)__builtin_amdgcn_kernarg_segment_ptr();   // (the block is the kernel's first argument: offset 0)
      asm volatile("" : "+s"(ka));
      // The hits of a run mostly lie in ONE instance: then the fields of its record that shading reads are read once for the wave, through the
      // scalar cache, and no row fetches them.  Otherwise a lane fetches the record of its own hit, and again only when a later row's differs.
      ShadeCarry carry;
      {
        int first = -1; bool agree = true;
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) {
          const int ij = (alive >> j) & 1u ? __float_as_int(bst[(4u * j + 3u) * 64u]) : -1;
          if (ij >= 0) { agree = agree && (first < 0 || ij == first); if (first < 0) first = ij; }
        }
        const uint64_t m_hit = __ballot(first >= 0);
        if (m_hit != 0ull) {
          const int one = __builtin_amdgcn_readlane(first, (int)__builtin_ctzll(m_hit));
          if (__ballot(first >= 0 && !(agree && first == one)) == 0ull) carry.set_instance(one, ShadeCarry::fields_of(ld_const(ld_const_ptr(&ka->sc.inst) + one)));
        }
      }
      asm volatile("" : "+s"(ka));   // (what follows is read after that: the record's words and the words below need not be in scalar registers together)
      const BeamShadeFrame sf{{{const_cast<float4* const*>(&ka->ray_o), nullptr}, {&ka->next_o, nullptr}},
                              {{nullptr, const_cast<float4*>(ld_const_ptr(&ka->ray_d))}, {&ka->next_d, nullptr}},
                              {&ka->sh_o, nullptr}, {&ka->sh_d, nullptr}, {&ka->sh_c, nullptr}, {&ka->sh_e, nullptr},
                              {nullptr, ld_const_ptr(&ka->sample_color)}, {nullptr, ld_const_ptr(&ka->counters)}, {&ka->light_entry, nullptr},
                              ld_const(&ka->shard_cap), ld_const(&ka->width), ld_const(&ka->rows), ld_const(&ka->light_tiles), ld_const(&ka->settle_dead_shadow_rays)};
      const BeamShadeScene sg{ka, ld_const(&ka->sc.n_materials), {&ka->sc.materials, nullptr}, {&ka->sc.prim_material, nullptr}};
      const BeamShadeUniforms su = ld_const(&ka->u);
      const BeamShadeView sv{sg, sf, su};
#pragma nounroll
      for (uint32_t j = 0; j < S; j++) {
        const float tj = j == 0u ? bt0 : (j == 1u ? bt1 : (j == 2u ? bt2 : bt3));
        const float* const b = bst + 256u * j;   // rows 4 j .. 4 j + 3
        const int ij = (alive >> j) & 1u ? __float_as_int(b[192]) : HIT_DEAD;
        shade_slot<false, false, false, true>(sv, 0, run_shard, v0 + 64u * j, true, ij, make_float4(tj, b[0], b[64], b[128]), &carry);
      }
    } else {
    // ---- the hit records of the pixel's samples (a slot without a ray: HIT_DEAD)
#define RT_BEAM_OUT(j) if (j < S) { \
      const uint32_t v = v0 + 64u * j; \
      if (alive & (1u << j)) { \
        st_stream(&a.hit_a[v], make_float4(bt##j, bst[(4 * j + 0) * 64], bst[(4 * j + 1) * 64], bst[(4 * j + 2) * 64])); \
        st_stream(&a.hit_inst[v], __float_as_int(bst[(4 * j + 3) * 64])); \
      } else st_stream(&a.hit_inst[v], HIT_DEAD); }
    RT_BEAM_EACH(RT_BEAM_OUT)
#undef RT_BEAM_OUT
    }
  }
  if (COUNT) {
    for (int off = 32; off > 0; off >>= 1) {
      cnt_nodes += __shfl_down((unsigned long long)cnt_nodes, off);
      cnt_tris += __shfl_down((unsigned long long)cnt_tris, off);
    }
    if (lane == 0) {
      atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + CNT_NODE_VISITS), (unsigned long long)cnt_nodes);
      atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + CNT_TRI_TESTS), (unsigned long long)cnt_tris);
      atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + CNT_DIAG), (unsigned long long)diag_iters);
      atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + CNT_DIAG + 2), (unsigned long long)diag_busy);
      atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + CNT_DIAG + 4), (unsigned long long)(__builtin_readcyclecounter() - diag_t0));
    }
  }
}

#ifndef RT_BEAM_WAVES
#define RT_BEAM_WAVES 4   /* waves per SIMD k_beam is register-allocated for: four rays' directions and distances beside the beam's ray space need ~120 VGPRs */
#endif
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_BEAM_WAVES, RT_BEAM_WAVES))) void k_beam(TraceArgs a, uint32_t run) { beam_body<false>(a, run); }
__global__ __launch_bounds__(256) void k_beam_count(TraceArgs a, uint32_t run) { beam_body<true>(a, run); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_BEAM_WAVES, RT_BEAM_WAVES))) void k_beam_shade(BeamShadeArgs a, uint32_t run) { beam_body<false, true>(a, run); }

#ifdef RT_ALT_KERNELS   // k_beam_shadow measured slower: only in librt_mi355x_alt.so
// ------------------------------------------------------------------------------------------------
// k_beam_shadow: the SHADOW rays of a pixel's samples walked together (src/shader.rgen:107-129, any hit).
// The shadow rays of a frame all END at the light — within 0.01 of it: a ray starts 0.01 N off its surface point P and runs parallel
// to the line from P to the light, for exactly that distance.  Seen from the light they are a beam again: ray j is
// E_j + s r_j, r_j = -direction, E_j = its end point, and E_j = E* + e_j with E* the end point of the pixel's first ray and |e_j| small
// (measured per ray, not assumed: the samples of a pixel mostly see the same surface, so their end points almost coincide).  A point of ray j inside a box is a point of the common-origin ray E* + s r_j inside the box grown by |e_j| — so the
// beam test of k_beam applies with the planes moved outwards by delta = max_j |e_j| (per axis, through the instance's linear part):
// near values minus delta |1/r|, far values plus delta |1/r|.  Triangles are tested against every ray that is not yet known to be
// occluded with the canonical any-hit test in the ray's own parametrisation (origin at the surface, tmin, tmax = distance), so
// whether a ray is occluded is decided exactly as in k_trace<shadow>; the walk ends when all of the pixel's rays are.
// Queue layout: with pixel runs k_shade puts the shadow ray of a PRIMARY hit into the slot of that primary ray (sh_*[q], a zero
// direction where there is none): the runs of bounce queue 0 are the runs here.  Shadow rays of later bounces stay in the compact
// shadow queue (k_trace<shadow>), which lives FrameDev::sh_base entries up in the same arrays.
struct BeamShadowArgs {
  TraceArgs t;        // ray_o / ray_d = sh_o / sh_d, sh_c, sh_e, sample_color, entry = the records of the cube around the light (or NULL),
                      // tails = the run cursors of bounce queue 0, work = this kernel's own cursors
  float light[3];
  uint32_t run;
};
struct BeamSpaceW { F3 s0, s1, n0, n1, f0, f1; uint3 rot; };   // BeamSpace with separate offsets for near (n) and far (f) planes

__device__ __forceinline__ bool slab_beam_w(uint32_t wx, uint32_t wy, uint32_t wz, const BeamSpaceW& B, float tmin, float tlim, float& tn, float& tfo) {
  wx = __builtin_amdgcn_alignbit(wx, wx, B.rot.x); wy = __builtin_amdgcn_alignbit(wy, wy, B.rot.y); wz = __builtin_amdgcn_alignbit(wz, wz, B.rot.z);
  const float nx = (float)(wx & 0xFFFFu), fx = (float)(wx >> 16), ny = (float)(wy & 0xFFFFu), fy = (float)(wy >> 16), nz = (float)(wz & 0xFFFFu), fz = (float)(wz >> 16);
  const float x0 = fminf(__builtin_fmaf(nx, B.s0.x, B.n0.x), __builtin_fmaf(nx, B.s1.x, B.n1.x)), x1 = fmaxf(__builtin_fmaf(fx, B.s0.x, B.f0.x), __builtin_fmaf(fx, B.s1.x, B.f1.x));
  const float y0 = fminf(__builtin_fmaf(ny, B.s0.y, B.n0.y), __builtin_fmaf(ny, B.s1.y, B.n1.y)), y1 = fmaxf(__builtin_fmaf(fy, B.s0.y, B.f0.y), __builtin_fmaf(fy, B.s1.y, B.f1.y));
  const float z0 = fminf(__builtin_fmaf(nz, B.s0.z, B.n0.z), __builtin_fmaf(nz, B.s1.z, B.n1.z)), z1 = fmaxf(__builtin_fmaf(fz, B.s0.z, B.f0.z), __builtin_fmaf(fz, B.s1.z, B.f1.z));
  tn = fmaxf(fmaxf(x0, y0), fmaxf(z0, tmin));
  const float tf = fminf(fminf(x1, y1), fminf(z1, tlim));
  tfo = tf;
  return tn <= tf * 1.00002f + 1.0e-6f;   // (the parameter starts at 0 here: an absolute slack beside the relative one)
}
// one axis: reciprocal directions lo <= hi, largest |direction| da, delta = how far the rays' own origins lie from the common one
__device__ __forceinline__ void beam_axis_w(float lo, float hi, float da, float t_far, float delta, float q_lo_minus_o, float q_scale,
                                            float& s0, float& s1, float& n0, float& n1, float& f0, float& f1, uint32_t& rot) {
  if (lo < 0.0f && hi > 0.0f) {
    const float K = 1.0e30f, inv = 1.0f / q_scale, r = __builtin_fmaf(t_far, da, delta);
    const float U = (r - q_lo_minus_o) * inv + 1.0f, L = (-r - q_lo_minus_o) * inv - 1.0f;
    s0 = K; s1 = K; n0 = -K * U; f0 = n0; n1 = -K * L; f1 = n1; rot = 0u;
  } else {
    s0 = q_scale * lo; s1 = q_scale * hi;
    const float b0 = q_lo_minus_o * lo, b1 = q_lo_minus_o * hi, e0 = delta * __builtin_fabsf(lo), e1 = delta * __builtin_fabsf(hi);
    n0 = b0 - e0; n1 = b1 - e1; f0 = b0 + e0; f1 = b1 + e1;
    rot = lo < 0.0f ? 16u : 0u;
  }
}

template <bool COUNT>
__device__ __forceinline__ void beam_shadow_body(const BeamShadowArgs& A) {
  const TraceArgs& a = A.t;
  __shared__ int s_stack[4][STACK2_LDS + 1][64];
  __shared__ float s_ray[4][24][64];     // ray j of lane l in the current space: rows 6 j .. 6 j + 5 = origin, direction (as k_trace's to_instance makes them)
  __shared__ float4 s_inst[LDS_INSTANCES ? LDS_INSTANCES : 1][5];
  const int n_lds_inst = a.sc.n_inst < LDS_INSTANCES ? a.sc.n_inst : LDS_INSTANCES;
  if ((int)threadIdx.x < n_lds_inst) {
    const InstanceDev* I = a.sc.inst + threadIdx.x;
    const float4* mp = reinterpret_cast<const float4*>(I->w2o);
    s_inst[threadIdx.x][0] = mp[0]; s_inst[threadIdx.x][1] = mp[1]; s_inst[threadIdx.x][2] = mp[2];
    s_inst[threadIdx.x][3] = make_float4(I->q_lo[0], I->q_lo[1], I->q_lo[2], __int_as_float(I->blas_root));
    s_inst[threadIdx.x][4] = make_float4(I->q_scale[0], I->q_scale[1], I->q_scale[2], __uint_as_float(I->mask));
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  int* const stk = &s_stack[wave][0][lane];
  float* const ray = &s_ray[wave][0][lane];                 // row r at ray[r * 64]
  const char* const node_bytes = reinterpret_cast<const char*>(a.sc.blas_nodes);
  const uint32_t S = A.run >> 6;
  uint64_t cnt_nodes = 0, cnt_tris = 0, diag_iters = 0, diag_busy = 0;   // (counting builds: trips of the interior loop, lanes busy in them)
  const uint64_t diag_t0 = COUNT ? __builtin_readcyclecounter() : 0;
  uint32_t shard = blockIdx.x & (N_SHARDS - 1), tried = 0;

  for (;;) {
    // ---- the wave's next run (wave-uniform); lane l walks the shadow rays of pixel l
    uint32_t base = 0; bool got = false;
    while (tried < (uint32_t)N_SHARDS) {
      const uint32_t size = ld_cursor(a.tails + shard * CNT_STRIDE);
      uint32_t off = 0;
      if (lane == 0 && size) off = atomicAdd(a.work + shard * CNT_STRIDE, A.run);
      off = (uint32_t)__builtin_amdgcn_readfirstlane((int)off);
      if (size && off < size) { base = shard * a.shard_cap + off; got = true; break; }
      shard = (shard + 1u) & (N_SHARDS - 1); tried++;
    }
    if (!got) break;
    const uint32_t v0 = base + lane;
    // which of the pixel's samples have a shadow ray, and how long it is
    uint32_t alive = 0, occluded = 0;
    float dt0 = -1.0f, dt1 = -1.0f, dt2 = -1.0f, dt3 = -1.0f;   // tmax of the ray (its distance to the light); no ray: never tested
#define RT_BEAM_ALIVE(j) if (j < S) { const float4 r = ld_stream(&a.ray_d[v0 + 64u * j]); if (r.x != 0.0f || r.y != 0.0f || r.z != 0.0f) { alive |= 1u << j; dt##j = ld_stream(&a.ray_o[v0 + 64u * j]).w; } }
    RT_BEAM_EACH(RT_BEAM_ALIVE)
#undef RT_BEAM_ALIVE
    // The samples of a pixel do not always see the same surface (a silhouette: one ray starts on the mesh in front, the next on the floor
    // behind it).  Rays that leave the light in directions far apart make a wide beam that touches half the tree, so a pixel is walked
    // in GROUPS of rays whose directions agree closely: `grp` is the group being walked, `todo` what is left.
    uint32_t todo = alive, grp = 0;
    BeamSpaceW B;
    B.s0 = B.s1 = B.n0 = B.n1 = B.f0 = B.f1 = mk3(0, 0, 0); B.rot = make_uint3(0u, 0u, 0u);
    int cur = REF_DONE, sp = 1, cur_inst = -1;
    auto push = [&](int v) {
      if (sp < STACK2_LDS) stk[sp * 64] = v;
      else *reinterpret_cast<volatile int32_t*>(a.ovf_stack + (size_t)(blockIdx.x * 256u + threadIdx.x) * a.sc.ovf_stride + (sp - STACK2_LDS)) = v;
      sp++;
    };
    auto pop = [&]() {
      sp--;
      if (sp < STACK2_LDS) cur = stk[sp * 64];
      else cur = *reinterpret_cast<volatile int32_t*>(a.ovf_stack + (size_t)(blockIdx.x * 256u + threadIdx.x) * a.sc.ovf_stride + (sp - STACK2_LDS));
    };
    // the live rays and their beam in the space of instance ii (ii < 0: the world).  Rays: exactly k_trace's (xform_point / xform_vec of
    // the world ray, t preserved) into LDS.  Beam: from the light; every ray's end point is measured against it (delta).
    auto set_space = [&](int ii, int& root, uint32_t& imask) {
      float qlo3[3] = {a.sc.tlas_q_lo[0], a.sc.tlas_q_lo[1], a.sc.tlas_q_lo[2]}, qsc3[3] = {a.sc.tlas_q_scale[0], a.sc.tlas_q_scale[1], a.sc.tlas_q_scale[2]};
      float m[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
      root = 0; imask = 0xFFu;
      if (ii >= 0) {
        float4 m0, m1, m2, ql, qsc;
        if (ii < n_lds_inst) { m0 = s_inst[ii][0]; m1 = s_inst[ii][1]; m2 = s_inst[ii][2]; ql = s_inst[ii][3]; qsc = s_inst[ii][4]; }
        else {
          const InstanceDev* I = a.sc.inst + ii;
          const float4* mp = reinterpret_cast<const float4*>(I->w2o);
          m0 = mp[0]; m1 = mp[1]; m2 = mp[2];
          ql = make_float4(I->q_lo[0], I->q_lo[1], I->q_lo[2], __int_as_float(I->blas_root));
          qsc = make_float4(I->q_scale[0], I->q_scale[1], I->q_scale[2], __uint_as_float(I->mask));
        }
        root = __float_as_int(ql.w); imask = __float_as_uint(qsc.w);
        if ((imask & 0xFFu) == 0u) return;
        m[0] = m0.x; m[1] = m0.y; m[2] = m0.z; m[3] = m0.w; m[4] = m1.x; m[5] = m1.y; m[6] = m1.z; m[7] = m1.w;
        m[8] = m2.x; m[9] = m2.y; m[10] = m2.z; m[11] = m2.w;
        qlo3[0] = ql.x; qlo3[1] = ql.y; qlo3[2] = ql.z; qsc3[0] = qsc.x; qsc3[1] = qsc.y; qsc3[2] = qsc.z;
      }
      float lx = 3.0e38f, ly = 3.0e38f, lz = 3.0e38f, hx = -3.0e38f, hy = -3.0e38f, hz = -3.0e38f, ax = 0.0f, ay = 0.0f, az = 0.0f, l2 = 3.0e38f;
      float dmax = 0.0f;
      F3 E0 = mk3(0, 0, 0), E1 = E0, E2 = E0, E3 = E0;
#define RT_BEAM_RAY(j) if (grp & (1u << j)) { \
        const float4 o4 = a.ray_o[v0 + 64u * j], d4 = a.ray_d[v0 + 64u * j]; \
        const F3 wo = mk3(o4.x, o4.y, o4.z), wd = mk3(d4.x, d4.y, d4.z); \
        const F3 co = ii >= 0 ? xform_point(m, wo) : wo, cd = ii >= 0 ? xform_vec(m, wd) : wd; \
        ray[(6 * j + 0) * 64] = co.x; ray[(6 * j + 1) * 64] = co.y; ray[(6 * j + 2) * 64] = co.z; \
        ray[(6 * j + 3) * 64] = cd.x; ray[(6 * j + 4) * 64] = cd.y; ray[(6 * j + 5) * 64] = cd.z; \
        E##j = fma3(o4.w, cd, co);   /* the reversed ray: from its end point E = co + tmax cd back along -cd */ \
        const float ix = safe_rcp(-cd.x), iy = safe_rcp(-cd.y), iz = safe_rcp(-cd.z); \
        lx = fminf(lx, ix); hx = fmaxf(hx, ix); ly = fminf(ly, iy); hy = fmaxf(hy, iy); lz = fminf(lz, iz); hz = fmaxf(hz, iz); \
        ax = fmaxf(ax, __builtin_fabsf(cd.x)); ay = fmaxf(ay, __builtin_fabsf(cd.y)); az = fmaxf(az, __builtin_fabsf(cd.z)); l2 = fminf(l2, dot3(cd, cd)); \
        dmax = fmaxf(dmax, o4.w); }
      RT_BEAM_EACH(RT_BEAM_RAY)
#undef RT_BEAM_RAY
      // the common origin of the beam: the end point of the group's first ray (the rays of a pixel end 0.01 N off the light with
      // almost the same N: far closer to each other than to the light); the others are measured against it
      const F3 eo = (grp & 1u) ? E0 : ((grp & 2u) ? E1 : ((grp & 4u) ? E2 : E3));
      float dx = 0.0f, dy = 0.0f, dz = 0.0f;
#define RT_BEAM_DEV(j) if (grp & (1u << j)) { dx = fmaxf(dx, __builtin_fabsf(E##j.x - eo.x)); dy = fmaxf(dy, __builtin_fabsf(E##j.y - eo.y)); dz = fmaxf(dz, __builtin_fabsf(E##j.z - eo.z)); }
      RT_BEAM_EACH(RT_BEAM_DEV)
#undef RT_BEAM_DEV
      // (the end points are evaluated in binary32: a relative allowance for their own rounding — and that of the boxes' planes against them — on top)
      const float slack = 4.0e-6f * (__builtin_fabsf(eo.x) + __builtin_fabsf(eo.y) + __builtin_fabsf(eo.z) + dmax * __builtin_sqrtf(fmaxf(ax * ax + ay * ay + az * az, 0.0f)));
      dx = __builtin_fmaf(dx, 1.01f, slack); dy = __builtin_fmaf(dy, 1.01f, slack); dz = __builtin_fmaf(dz, 1.01f, slack);
      const float ex = fmaxf(__builtin_fabsf(qlo3[0] - eo.x), __builtin_fabsf(__builtin_fmaf(65535.0f, qsc3[0], qlo3[0]) - eo.x));
      const float ey = fmaxf(__builtin_fabsf(qlo3[1] - eo.y), __builtin_fabsf(__builtin_fmaf(65535.0f, qsc3[1], qlo3[1]) - eo.y));
      const float ez = fmaxf(__builtin_fabsf(qlo3[2] - eo.z), __builtin_fabsf(__builtin_fmaf(65535.0f, qsc3[2], qlo3[2]) - eo.z));
      const float t_far = fminf(dmax * 1.001f, 1.001f * (__builtin_sqrtf((ex * ex + ey * ey + ez * ez) / fmaxf(l2, 1.0e-30f)) + (dx + dy + dz) * 1.0e3f + 1.0e-3f));   /* (+ the rays' own offsets from the common origin, generously) */
      beam_axis_w(lx, hx, ax, t_far, dx, qlo3[0] - eo.x, qsc3[0], B.s0.x, B.s1.x, B.n0.x, B.n1.x, B.f0.x, B.f1.x, B.rot.x);
      beam_axis_w(ly, hy, ay, t_far, dy, qlo3[1] - eo.y, qsc3[1], B.s0.y, B.s1.y, B.n0.y, B.n1.y, B.f0.y, B.f1.y, B.rot.y);
      beam_axis_w(lz, hz, az, t_far, dz, qlo3[2] - eo.z, qsc3[2], B.s0.z, B.s1.z, B.n0.z, B.n1.z, B.f0.z, B.f1.z, B.rot.z);
    };

    // the next group of the pixel's rays, and the start of its walk: at the record of the group's tile of the cube around the light when
    // its rays agree on one (k_shade wrote it per ray), at the root of the TLAS otherwise
    auto next_group = [&]() {
      F3 w0 = mk3(0, 0, 0), w1 = w0, w2 = w0, w3 = w0;
#define RT_BEAM_LD(j) if (todo & (1u << j)) { const float4 r = a.ray_d[v0 + 64u * j]; w##j = mk3(r.x, r.y, r.z); }
      RT_BEAM_EACH(RT_BEAM_LD)
#undef RT_BEAM_LD
      const F3 wf = (todo & 1u) ? w0 : ((todo & 2u) ? w1 : ((todo & 4u) ? w2 : w3));
      grp = 0;
#define RT_BEAM_GRP(j) if ((todo & (1u << j)) && fmaxf(fmaxf(__builtin_fabsf(w##j.x - wf.x), __builtin_fabsf(w##j.y - wf.y)), __builtin_fabsf(w##j.z - wf.z)) <= 0.01f) grp |= 1u << j;
      RT_BEAM_EACH(RT_BEAM_GRP)
#undef RT_BEAM_GRP
      todo &= ~grp;
      uint32_t ent = 0xFFFFFFFEu;
#define RT_BEAM_ENT(j) if (grp & (1u << j)) { const uint32_t e = a.entry != nullptr ? (a.sh_e[v0 + 64u * j] & ~ENTRY_REVERSE) : ENTRY_FROM_ROOT; ent = (ent == 0xFFFFFFFEu || ent == e) ? e : ENTRY_FROM_ROOT; }
      RT_BEAM_EACH(RT_BEAM_ENT)
#undef RT_BEAM_ENT
      stk[0] = REF_DONE; sp = 1; cur = REF_DONE; cur_inst = -1;
      int root; uint32_t imask;
      if (ent == ENTRY_FROM_ROOT) { set_space(-1, root, imask); cur = a.sc.tlas_root; }
      else {
        const int4* rp = reinterpret_cast<const int4*>(a.entry + ent);
        const int4 r0 = rp[0], r1 = rp[1];
        const uint32_t hdr = (uint32_t)r0.x;
        if (hdr != ENTRY_EMPTY) {   // (empty: nothing between this tile of the cube and the light: the group's rays are lit)
          const uint32_t nw = hdr & 15u, ia = hdr >> 8;
          const int wk[6] = {r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
          for (uint32_t k = 0; k < 6u; k++) if (k < nw) stk[(1u + k) * 64u] = wk[k];
          sp = 1 + (int)nw;
          cur = r0.y;
          if (ia != ENTRY_NO_INST) { set_space((int)ia, root, imask); cur_inst = (int)ia; }
          else set_space(-1, root, imask);
        }
      }
    };
    stk[0] = REF_DONE;
    typedef __attribute__((address_space(3))) volatile int lds_vint;
    lds_vint* const stk_lds = (lds_vint*)stk;
    for (;;) {
      if (cur == REF_DONE && todo != 0u) next_group();   // (a group is done, or the pixel begins)
      const uint32_t live = (uint32_t)__builtin_popcountll(__ballot(cur != REF_DONE || todo != 0u));
      if (live == 0u) break;
      const uint32_t keep_going = (live * RT_KEEP_NUM + 7u) >> 3;
      for (;;) {
        const uint32_t n_int = (uint32_t)__builtin_popcountll(__ballot(cur >= 0));
        if (n_int == 0u || n_int < keep_going) break;
        if (COUNT && lane == 0) { diag_iters++; diag_busy += n_int; }
        // the parameter runs from the light (0) to the surface: no ray reaches beyond the longest one of the group that is still undecided
        const uint32_t und = grp & ~occluded;
        const float tlim = 1.0001f * fmaxf(fmaxf((und & 1u) ? dt0 : -1.0f, (und & 2u) ? dt1 : -1.0f), fmaxf((und & 4u) ? dt2 : -1.0f, (und & 8u) ? dt3 : -1.0f));
        const bool deep = cur >= 0 && sp + RT_INTERIOR_UNROLL > STACK2_LDS;
        if (__ballot(deep) == 0ull) {
#pragma unroll
          for (int r = 0; r < RT_INTERIOR_UNROLL; r++)
            if (cur >= 0) {
              const uint4* np = reinterpret_cast<const uint4*>(node_bytes + ((uint32_t)cur << 5));
              const uint4 Q0 = np[0], Q1 = np[1];
              const int top = stk_lds[(sp - 1) * 64];
              const int2 ch = make_int2((int)Q1.z, (int)Q1.w);
              if (COUNT) cnt_nodes++;
              float t0, t1, f0, f1;
              const bool h0 = slab_beam_w(Q0.x, Q0.y, Q0.z, B, -1.0e-3f, tlim, t0, f0);
              const bool h1 = slab_beam_w(Q0.w, Q1.x, Q1.y, B, -1.0e-3f, tlim, t1, f1);
              // the child that reaches FARTHER from the light first: an occluder near the surface is the likely one
              const bool both = h0 && h1, none = !(h0 || h1), swap = f1 > f0;
              const uint32_t pm = 0u - (uint32_t)both;
              stk_lds[(((uint32_t)sp & pm) | ((uint32_t)STACK2_LDS & ~pm)) * 64u] = swap ? ch.x : ch.y;
              const int one = h0 ? ch.x : ch.y;
              cur = both ? (swap ? ch.y : ch.x) : (none ? top : one);
              sp += (both ? 1 : 0) - (none ? 1 : 0);
            }
        } else {
#pragma unroll
          for (int r = 0; r < RT_INTERIOR_UNROLL; r++)
            if (cur >= 0) {
              const uint4* np = reinterpret_cast<const uint4*>(node_bytes + ((uint32_t)cur << 5));
              const uint4 Q0 = np[0], Q1 = np[1];
              const int2 ch = make_int2((int)Q1.z, (int)Q1.w);
              if (COUNT) cnt_nodes++;
              float t0, t1, f0, f1;
              const bool h0 = slab_beam_w(Q0.x, Q0.y, Q0.z, B, -1.0e-3f, tlim, t0, f0);
              const bool h1 = slab_beam_w(Q0.w, Q1.x, Q1.y, B, -1.0e-3f, tlim, t1, f1);
              if (h0 && h1) { const bool swap = f1 > f0; push(swap ? ch.x : ch.y); cur = swap ? ch.y : ch.x; }
              else if (h0) cur = ch.x;
              else if (h1) cur = ch.y;
              else pop();
            }
        }
      }
      // BLAS leaf: the canonical any-hit test (src/shader.rgen:110-112: tmin 0.001, tmax the distance) of every ray still undecided
      if (cur < 0 && cur > REF_MARK && cur_inst >= 0) {
        const uint32_t ref = (uint32_t)(~cur);
        const uint32_t first = ref >> 3, count = (ref & 7u) + 1u;
        for (uint32_t k = 0; k < count; k++) {
          const float4* tp = a.sc.tris + (size_t)(first + k) * 3;
          const float4 T0 = tp[0], T1 = tp[1], T2 = tp[2];
#define RT_BEAM_TRI(j) if ((grp & ~occluded) & (1u << j)) { \
            if (COUNT) cnt_tris++; \
            const F3 co = mk3(ray[(6 * j + 0) * 64], ray[(6 * j + 1) * 64], ray[(6 * j + 2) * 64]), cd = mk3(ray[(6 * j + 3) * 64], ray[(6 * j + 4) * 64], ray[(6 * j + 5) * 64]); \
            float tt, uu, vv; \
            if (tri_test(T0, T1, T2, co, cd, a.tmin, dt##j, tt, uu, vv)) occluded |= 1u << j; }
          RT_BEAM_EACH(RT_BEAM_TRI)
#undef RT_BEAM_TRI
        }
        if ((grp & ~occluded) == 0u) cur = REF_DONE;   // every ray of the group has its answer (flags 13, src/shader.rgen:67: the first hit ends a ray)
        else pop();
      }
      if (cur == REF_MARK) {
        cur_inst = -1;
        pop();
        if (cur >= 0) { int root; uint32_t imask; set_space(-1, root, imask); }
      }
      if (cur < 0 && cur > REF_MARK && cur_inst < 0) {
        const int ii = ~cur;
        int root; uint32_t imask;
        set_space(ii, root, imask);
        if ((imask & 0xFFu) == 0u) {
          pop();
          if (cur >= 0) set_space(-1, root, imask);
        } else {
          push(REF_MARK);
          cur_inst = ii; cur = root;
        }
      }
    }
    // ---- src/shader_shadow.rmiss:6 + src/shader.rgen:114-129, as k_trace<shadow>'s epilogue: the lit colour of the queue entry, or Iamb*ka
#define RT_BEAM_OUT(j) if (alive & (1u << j)) { \
      const uint32_t v = v0 + 64u * j; \
      const bool lit = (occluded & (1u << j)) == 0u; \
      float cr = 0.08f, cg = 0.24f, cb = 0.08f; \
      if (lit || a.sc.n_materials != 0) { \
        const float4 shc = ld_stream(&a.sh_c[v]); \
        if (lit) { cr = shc.x; cg = shc.y; cb = shc.z; } \
        else { const F3 amb = ambient_of(a.sc, __float_as_uint(shc.w)); cr = amb.x; cg = amb.y; cb = amb.z; } \
      } \
      st_stream(&a.sample_color[__float_as_uint(ld_stream(&a.ray_d[v]).w)], make_float4(cr, cg, cb, 1.0f)); }
    RT_BEAM_EACH(RT_BEAM_OUT)
#undef RT_BEAM_OUT
  }
  if (COUNT) {
    for (int off = 32; off > 0; off >>= 1) {
      cnt_nodes += __shfl_down((unsigned long long)cnt_nodes, off);
      cnt_tris += __shfl_down((unsigned long long)cnt_tris, off);
    }
    if (lane == 0) {
      atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + CNT_NODE_VISITS_SH), (unsigned long long)cnt_nodes);
      atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + CNT_TRI_TESTS_SH), (unsigned long long)cnt_tris);
      atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + CNT_DIAG_SH), (unsigned long long)diag_iters);
      atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + CNT_DIAG_SH + 2), (unsigned long long)diag_busy);
      atomicAdd(reinterpret_cast<unsigned long long*>(a.counters + CNT_DIAG_SH + 4), (unsigned long long)(__builtin_readcyclecounter() - diag_t0));
    }
  }
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_BEAM_WAVES, RT_BEAM_WAVES))) void k_beam_shadow(BeamShadowArgs a) { beam_shadow_body<false>(a); }
__global__ __launch_bounds__(256) void k_beam_shadow_count(BeamShadowArgs a) { beam_shadow_body<true>(a); }
#endif  // RT_ALT_KERNELS
