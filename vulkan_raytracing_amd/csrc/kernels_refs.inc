// kernels_refs.inc — included by kernels.hip after kernels_triangle.inc (product and alt translation units alike).
// rt_scene_triangles_device, rt_overlap_scene_triangles_device, rt_closest_scene_triangle_device: the two triangle queries asked about
// triangles of the scene itself, named by (inst, prim) references (rt_tri_ref, 16 bytes: inst, prim, against, r_max).
//
//  * k_refs_expand, one thread per reference, writes the 48-byte record of the plain triangle calls: the world image of the source
//    packet in the arithmetic the candidate side uses (v0, e1 = v1 - v0, e2 = v2 - v0 rounded once; P0 = xform_point(o2w, v0),
//    P1 = P0 + xform_vec(o2w, e1), P2 = P0 + xform_vec(o2w, e2): collide_tri's (A, B, C) of that instance and packet), r_max in word 3,
//    the bits of inst in word 7 and of against in word 11.  An invalid reference gets nine quiet NaNs, which both walks answer as they
//    answer any record with a non-finite vertex.  Nothing of the scene is indexed with an unchecked value: inst, then against, then prim
//    against the triangle count of the instance's mesh (InstanceDev::prim_count), then the loads;
//  * the walks are the REFS instantiations of overlap_body and nearest_body (walk_overlap.inc, walk_nearest.inc) with the triangle
//    shapes (kernels_triangles.inc, kernels_triangle.inc) over the expanded records, under kernel names of their own.

// The world image (P0, P1, P2) of triangle `prim` of instance I (a checked instance of the scene), or nothing: prim outside the mesh, a
// bad triangle, an image that is not finite.  k_refs_expand's loads, checks and arithmetic, which the instance-pair walks
// (kernels_pairs.inc) repeat for their work items: one function, so that both make the same bytes.
__device__ __forceinline__ bool refs_world_triangle(const SceneDev& sc, const InstanceDev* I, int prim, uint32_t n_vert_floats, F3& P0, F3& P1, F3& P2) {
  bool made = false;
  {
    if (prim >= 0 && (uint32_t)prim < I->prim_count) {
      const uint32_t* ip = sc.idx + I->first_index + 3ull * (uint32_t)prim;
      const uint32_t i0 = ip[0], i1 = ip[1], i2 = ip[2];
      const uint64_t top = (uint64_t)I->first_float + 6ull * max(max(i0, i1), i2) + 3u;   // (rt_upload_geometry checked the indices: always true)
      if (top <= n_vert_floats) {
        const float* vb = sc.verts + I->first_float;
        const float* p0 = vb + 6ull * i0;
        const float* p1 = vb + 6ull * i1;
        const float* p2 = vb + 6ull * i2;
        const F3 v0 = mk3(p0[0], p0[1], p0[2]), v1 = mk3(p1[0], p1[1], p1[2]), v2 = mk3(p2[0], p2[1], p2[2]);
        // a BAD TRIANGLE (rt_upload_geometry): a coordinate that is not finite or of magnitude BAD_COORD_LIMIT or more
        const float big = fmaxf(fmaxf(fmaxf(fmaxf(__builtin_fabsf(v0.x), __builtin_fabsf(v0.y)), __builtin_fabsf(v0.z)),
                                      fmaxf(fmaxf(__builtin_fabsf(v1.x), __builtin_fabsf(v1.y)), __builtin_fabsf(v1.z))),
                                fmaxf(fmaxf(__builtin_fabsf(v2.x), __builtin_fabsf(v2.y)), __builtin_fabsf(v2.z)));
        const bool good = finite_bits(v0.x) && finite_bits(v0.y) && finite_bits(v0.z) && finite_bits(v1.x) && finite_bits(v1.y) && finite_bits(v1.z) &&
                          finite_bits(v2.x) && finite_bits(v2.y) && finite_bits(v2.z) && big < BAD_COORD_LIMIT;
        const F3 A = xform_point(I->o2w, v0);
        const F3 B = add3(A, xform_vec(I->o2w, sub3(v1, v0))), Cc = add3(A, xform_vec(I->o2w, sub3(v2, v0)));
        if (good && finite_bits(A.x) && finite_bits(A.y) && finite_bits(A.z) && finite_bits(B.x) && finite_bits(B.y) && finite_bits(B.z) &&
            finite_bits(Cc.x) && finite_bits(Cc.y) && finite_bits(Cc.z)) {
          P0 = A; P1 = B; P2 = Cc; made = true;
        }
      }
    }
  }
  return made;
}

__global__ __launch_bounds__(256) void k_refs_expand(SceneDev sc, const int4* __restrict__ refs, float4* __restrict__ out, uint32_t n, uint32_t n_vert_floats) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int4 r = refs[i];
  const int inst = r.x, prim = r.y, against = r.z;
  const float QNAN = __uint_as_float(0x7FC00000u);
  F3 P0 = mk3(QNAN, QNAN, QNAN), P1 = P0, P2 = P0;
  if (inst >= 0 && inst < sc.n_inst && against >= -1 && against < sc.n_inst) refs_world_triangle(sc, sc.inst + inst, prim, n_vert_floats, P0, P1, P2);
  float4* o = out + 3u * (size_t)i;
  o[0] = make_float4(P0.x, P0.y, P0.z, __int_as_float(r.w));
  o[1] = make_float4(P1.x, P1.y, P1.z, __int_as_float(inst));
  o[2] = make_float4(P2.x, P2.y, P2.z, __int_as_float(against));
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_refs_collide(OverlapArgs a) { overlap_body<OverlapTriangle, false, true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_OVERLAP_WAVES_PER_EU))) void k_refs_collide_count(OverlapArgs a) { overlap_body<OverlapTriangle, true, true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_TRIANGLE_WAVES_PER_EU))) void k_refs_nearest(NearestArgs a) { nearest_body<NearestTriangle, false, true>(a); }
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_TRIANGLE_WAVES_PER_EU))) void k_refs_nearest_count(NearestArgs a) { nearest_body<NearestTriangle, true, true>(a); }

void launch_refs_expand(const SceneDev& sc, const void* refs, float4* tris, uint32_t n, uint64_t n_vert_floats, hipStream_t s) {
  const uint32_t cap = (uint32_t)(n_vert_floats < 0xFFFFFFFFull ? n_vert_floats : 0xFFFFFFFFull);
  hipLaunchKernelGGL(k_refs_expand, dim3((n + 255u) / 256u), dim3(256), 0, s, sc, (const int4*)refs, tris, n, cap);
}
