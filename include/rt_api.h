/* rt_api.h — C ABI of librt_mi355x.so, the MI355X (gfx950) replacement for the reference's
 * VK_KHR_ray_tracing_pipeline stage.
 *
 * The reference (mcan1999/vulkan-raytracing) reaches its ray-tracing stage through raw Vulkan calls
 * inlined in main(); it has no plugin/FFI interface.  This header cuts the seam at the Vulkan
 * objects the host creates for that stage: one export per Vulkan interaction on the path.  Each
 * declaration cites the reference call site it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every call returns 0 on success (mirrors VK_SUCCESS); non-zero = rt_status below, message via
 *     rt_last_error().  No exception crosses the boundary (the reference throws
 *     std::runtime_error("Vulkan API exception...") from throwExceptionVulkanAPI, src/main.cpp:138-147;
 *     the C++ host wrapper host/rt_host.hpp re-throws to keep that behaviour).
 *   - the caller owns every host array; the library copies on upload (as copyData does,
 *     src/main.cpp:203-219).  Handles are opaque; destroy is explicit.
 *   - one context drives one GPU and is not re-entrant (the reference is single-threaded with one
 *     queue and a blocking fence after every build/upload); the contexts of one scene family (rt_create_frame_slot)
 *     are driven from one host thread as well.
 *   - plain pointers and sizes only; no torch / HIP types in signatures (streams are void*).
 */
#ifndef RT_API_H
#define RT_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_ctx rt_ctx;

enum rt_status {
  RT_OK = 0,
  RT_ERR_INVALID_ARGUMENT = 1,
  RT_ERR_NOT_READY = 2,      /* call order violated (e.g. trace before geometry/instances/uniforms) */
  RT_ERR_DEVICE = 3,         /* a HIP runtime call failed; see rt_last_error */
  RT_ERR_OUT_OF_MEMORY = 4,
  RT_ERR_NO_DEVICE = 5       /* no usable gfx950 device: the library never falls back to the CPU */
};

/* One object of the shared vertex/index buffers (generalises orbitingObjectVertexOffset /
 * orbitingObjectPrimitiveOffset, src/main.cpp:1872-1873). */
typedef struct rt_mesh_range {
  uint64_t first_float;   /* offset into verts6, in floats (= vertexOffset of src/shader.rchit:55) */
  uint64_t first_index;   /* offset into idx, in uint32s (= 3*primitiveOffset) */
  uint32_t prim_count;    /* triangles (src/main.cpp:1644) */
  uint32_t reserved;
} rt_mesh_range;

/* 64-byte mirror of VkAccelerationStructureInstanceKHR as filled by createInstance
 * (src/main.cpp:538-551): a maintainer can memcpy the Vulkan struct and overwrite the last field. */
typedef struct rt_instance {
  float transform[12];              /* row-major 3x4 object->world (glmToVulkan, src/main.cpp:245-249) */
  uint32_t custom_index_and_mask;   /* instanceCustomIndex:24 (low) | mask:8 (high) */
  uint32_t sbt_offset_and_flags;    /* instanceShaderBindingTableRecordOffset:24 | flags:8 (RT_INSTANCE_FLAG_*: read by
                                       rt_intersect_device_flags only; frames ignore them, as the reference, which always uses
                                       offset 0 / TRIANGLE_FACING_CULL_DISABLE) */
  uint64_t mesh;                    /* index into rt_mesh_range[] — replaces accelerationStructureReference.
                                       RULE: the closest-hit stage reads the index/vertex range of THIS mesh.  The reference
                                       picks the range from instanceCustomIndex instead (src/shader.rchit:52-58: index 0 -> no
                                       offset, otherwise the orbiting object's offsets), which is the same thing whenever
                                       customIndex k is given to instances of mesh k, as src/main.cpp:1810-1816 does; an
                                       instance of mesh 1 created with customIndex 0 would read the wrong triangles there and
                                       the right ones here.  customIndex still selects the material type (src/shader.rgen:96) */
} rt_instance;

/* The 104-byte UniformStructure, field for field (src/main.cpp:1847-1866; src/shader.rgen:22-46). */
typedef struct rt_uniforms {
  float position[4];
  float right[4];
  float up[4];
  float forward[4];
  float light_position[3];
  float light_intensity;
  uint32_t max_bounce_count;
  uint32_t samples_per_pixel;
  uint32_t center_object_type;      /* 0 diffuse, 1 mirror, 2 refractive (include/config.h:9-16) */
  uint32_t orbiting_object_type;
  uint32_t orbiting_object_primitive_offset;  /* informational: ranges[] is authoritative */
  uint32_t orbiting_object_vertex_offset;
} rt_uniforms;

/* Result of one traceRayEXT (src/shader.rgen:86-87 / 111-112): what the driver hands to rchit/rmiss. */
typedef struct rt_hit {
  float t, u, v;        /* gl_HitTEXT and hitAttributeEXT vec2 (barycentrics of vertices B, C) */
  int32_t prim;         /* gl_PrimitiveID; -1 on miss */
  int32_t inst;         /* index into the instance array (gl_InstanceID); -1 on miss */
} rt_hit;

typedef struct rt_stats {
  uint64_t rays_primary;     /* one count per traceRayEXT-equivalent, by class */
  uint64_t rays_secondary;
  uint64_t rays_shadow;
  uint64_t node_visits;      /* closest-hit kernel; filled only by the instrumented (counting) kernels */
  uint64_t tri_tests;
  uint64_t node_visits_shadow; /* any-hit kernel, same */
  uint64_t tri_tests_shadow;
  uint64_t diag[6];          /* counting build: loop trips, busy quad-trips, wave cycles (closest; shadow) */
  uint64_t closest_rays;     /* rays through the closest-hit traversal kernel (primary+secondary) */
  float ms_frame;            /* HIP-event time of the whole frame pipeline on the trace stream */
  float ms_raygen;
  float ms_trace_closest;    /* sum over its launches of the closest-hit traversal kernel k_trace (not k_tail) */
  float ms_trace_shadow;     /* any-hit traversal kernel */
  float ms_shade;
  float ms_resolve;
  uint32_t launches_trace_closest;   /* per frame */
  uint32_t launches_total;
  uint32_t timed_frames;     /* the ms_* fields are means over this many frames (all frames enqueued with timing on
                                since the previous rt_get_stats / rt_trace) */
  float ms_tail;             /* k_tail: bounces 1..maxBounceCount in one launch (0 when the per-bounce launches ran) */
  uint32_t bvh_node_bytes;   /* S_node, S_tri of the roofline formula */
  uint32_t bvh_tri_bytes;
  uint32_t tail_faults;      /* frames of this context that were rendered again with per-bounce launches because a k_tail grid
                                barrier gave up (its workgroups were not co-resident); the context stays off k_tail afterwards */
  uint32_t frames_rerendered; /* 1 when the frame these statistics belong to had to be rendered a second time (k_tail fault): a copy of
                                the frame taken BEFORE this call returned (a gather or memcpy enqueued behind rt_trace_shard) is stale */
  /* ABI 6 — tile blobs (rt_set_param "tile_blobs"): the nodes and triangle packets a screen tile's rays can touch, staged through LDS */
  uint64_t blob_tiles;          /* tiles of this frame whose primary rays were walked in LDS */
  uint64_t blob_tiles_large;    /* ... of which needed the large size class (counting builds fill the blob_* fields) */
  uint64_t blob_tiles_refused;  /* tiles whose blob fit no size class (nodes, packets, depth, arena): their rays took the global walk */
  uint64_t blob_nodes;          /* nodes / triangle packets in all blobs of the frame */
  uint64_t blob_tris;
  uint64_t tile_rays;           /* primary rays walked in LDS (part of closest_rays) */
  uint64_t tile_rays_handed_on; /* ... of which went on to the global walk because they could still hit another instance */
  uint64_t tile_diag[6];        /* counting builds: wave cycles of k_tile before the walk (blob copy, ray generation), in the walk, in all; then from the
                                   start of the workgroup until: its list entry is there, the blob is in LDS, the ray is set up */
  uint64_t rays_shadow_untraced; /* ABI 7 — of rays_shadow: shadow rays whose outcome cannot change their sample (the surface and the half vector face away from
                                    the light: diffuse and specular are exactly 0, src/shader.rgen:113-128) — settled in k_shade, not walked (rt_set_param "dead_shadow_rays") */
} rt_stats;

/* Device/queue/pipeline creation (src/main.cpp:928-1102, 1578-1601).  device_id = HIP ordinal. */
int rt_create(rt_ctx** out_ctx, int device_id);
/* A second (third, ...) frame in flight on the same GPU: a context that SHARES the parent's scene — geometry, BLAS, cube map,
 * everything rt_upload_geometry / rt_build_blas / rt_set_skybox created, before or after this call — and owns only what one
 * frame needs: its instance records and TLAS, its uniform block, its ray queues, counters and stream.  This is the
 * reference's per-swapchain-image state (command buffer, fence, semaphores: src/main.cpp:2597, 2740-2749) next to its
 * shared buffers and acceleration structures.  Scene-building calls on ANY context of the family wait for the frames of
 * all of them, rebuild the shared scene and invalidate every slot's TLAS (call rt_set_instances again).  At most 16
 * contexts share a scene; rt_destroy on the last one frees it. */
int rt_create_frame_slot(rt_ctx* parent, rt_ctx** out_ctx);
/* Cleanup (src/main.cpp:2977-3060). */
void rt_destroy(rt_ctx* ctx);

/* buildBuffer for the shared vertex and index buffers (src/main.cpp:1684-1697, 1713-1726).
 * verts6 = interleaved [px py pz nx ny nz] (src/main.cpp:1673-1682), idx = object-local uint32.
 *
 * Bad vertices (for rt_upload_geometry + rt_build_blas with every builder, the vertices on the host or, after a refit, on the device
 * only).  A vertex position is a caller-supplied input like an instance record (rt_set_instances, "bad records") and has its
 * degenerate forms specified: a NaN from a skinning kernel or an overflowed literal costs the triangles that name it and nothing else.
 *   BAD TRIANGLE: one of the nine position coordinates of its three vertices is not finite, or has magnitude >= 1e37 (the limit of an
 *     instance's box: a larger coordinate in the mesh bounds would void every instance of the mesh).  It is not an error:
 *     rt_upload_geometry and rt_build_blas return RT_OK.  A bad triangle is INACTIVE for every builder and every consumer: never hit,
 *     never a candidate of any query, and it adds nothing to any node box, to the mesh bounds, to the centroid bounds or to the
 *     dequantisation of the mesh.  Every other triangle keeps its primitive index, its material and its answers, bit for bit.
 *     A mesh whose triangles are all bad behaves like a mesh without triangles: its instances are never entered (rt_set_instances over
 *     them is RT_OK).  Normals are not part of this: a normal that is not finite changes the shading of its own hits only.
 *   FAR vertices: a finite coordinate below the limit (1e30) is valid.  The mesh answers bit for bit as over the vertices as they are,
 *     only more slowly (its boxes collapse into a few quanta); the closest hit does not depend on the tree.  Its
 *     instances are subject to the box limit of rt_set_instances like any other.
 *   rt_refit_blas_device keeps its rule: a position in the NEW vertices that is not finite is RT_ERR_INVALID_ARGUMENT and the mesh
 *     counts as not built.  A later rt_build_blas builds over those vertices under the rule above.  A refit with all-finite vertices
 *     over a mesh built with inactive triangles makes them active: frames and hits are those of a fresh build over the new vertices. */
int rt_upload_geometry(rt_ctx* ctx, const float* verts6, size_t n_floats, const uint32_t* idx, size_t n_idx,
                       const rt_mesh_range* ranges, int n_meshes);

/* createBLASGeometry + createBLAS + createBLASScratchBuffer + buildBLAS (src/main.cpp:305-536, called
 * :1734-1799).  Synchronous like the reference's fence wait (:525-527).  Bad vertex positions are no error: see rt_upload_geometry. */
int rt_build_blas(rt_ctx* ctx, int mesh);

/* createInstance + createTLAS (src/main.cpp:538-793; called :1818-1835 with update=false and every
 * frame :2848-2861 with update=true).  update!=0 keeps the TLAS topology and refits boxes (Vulkan
 * UPDATE mode, src=dst); it requires the same instance count as the last build.  Never waits for the frame in flight: the
 * instance records and TLAS nodes are double-buffered, the new set travels on the context's stream (pinned staging) and
 * the next frame is ordered behind it; only the frame before the last is waited for, if it is still running (the reference
 * allocates buffers and blocks on a fence here every frame, src/main.cpp:672-696, 752-778).
 *
 * Bad records (the same for rt_set_instances_device, whose records no host ever sees, and for every frame of rt_set_batch).  None of
 * them is an error — the call returns RT_OK — and none of them changes what any OTHER instance answers: every other instance keeps its
 * index, objectIndex, type and results, bit for bit.
 *   VOID record: one of the 12 transform entries is not finite (NaN, +-inf: a simulation that blew up, a 0xFF-filled slot), or the
 *     padded world box of the instance has a coordinate of magnitude >= 1e37 (a body that flew off; FLT_MAX / 34).  In every frame and
 *     every query the record behaves exactly like the same record with mask 0: never entered, never a candidate, whatever the cull
 *     mask.  It adds nothing to the TLAS bounds, the centroid bounds or the quantisation; its box is that of an empty mesh.
 *   NON-INVERTIBLE record: the transform is finite and its inverse (gl_WorldToObjectEXT, binary64 cofactors rounded once) has an entry
 *     that is not finite — a singular matrix (a flattened body, a zero-filled slot), a scale below about 3e-39 whose inverse overflows
 *     binary32.  No ray ever hits it: frames, rt_intersect*, rt_intersect_device_flags / _hits, rt_point_inside*, the vote of
 *     rt_signed_distance_device, rt_shade_rays_device.  The world-space queries (rt_closest_point*, rt_sweep_spheres*,
 *     rt_overlap_boxes*, rt_overlap_triangles*, rt_closest_segment*, rt_closest_triangle*) keep answering over the o2w image of its triangles, as their own sections say.
 *   FAR record: finite and below the limit (a translation of 1e30) is a VALID record.  Nothing is promised about hitting it (binary32
 *     has no resolution left out there, and the TLAS planes are 1e30 / 65530 apart); the rest of the scene answers bit for bit as
 *     without it, more slowly: the closest hit does not depend on the tree. */
int rt_set_instances(rt_ctx* ctx, const rt_instance* instances, int n, int update);

/* createTLAS with a DEVICE instance buffer (src/main.cpp:538-793: the reference's instance buffer is device memory and the TLAS is
 * built by the device).  d_instances = n rt_instance records (64 B each, same layout and rules as rt_set_instances) in memory of
 * ctx's GPU, read in stream order on hip_stream (NULL = the context's stream): the library copies them into its own buffer on that
 * stream, so the caller may overwrite its buffer with work queued on the same stream as soon as the call returns.  Everything else
 * happens on the device, on a build stream of the context that waits for hip_stream: the instance records (w2o bit-identical to
 * rt_set_instances'), an LBVH over the instance boxes (update = 0) or a bottom-up refit of the topology of this context's previous
 * rt_set_instances_device build (update != 0: same n), the quantised TLAS nodes.  The call returns once a small summary of the
 * build is back on the host (the reference waits on its fence inside createTLAS, :772-778); it does not wait for the frame in
 * flight: records and TLAS are double-buffered exactly as for rt_set_instances.  Frames and hit records are bit-identical to
 * those of rt_set_instances with the same records (the closest hit does not depend on the tree).
 * Void, non-invertible and far records are treated as rt_set_instances documents them, by the same two tests on the device: a record
 * a physics kernel left non-finite or singular costs the scene nothing but that record, in builds and in refits (a refit with the
 * record good again restores the state of the original build bit for bit).
 * 1 <= n <= 1048576.  RT_ERR_INVALID_ARGUMENT: a NULL pointer, n out of range, an unknown mesh index, trace_variant != 0, an
 * update whose previous build came from rt_set_instances / rt_set_batch (and an rt_set_instances update after this call);
 * RT_ERR_NOT_READY: an instance of a mesh whose BLAS is not built.  After an error the context's TLAS is invalid until the next
 * successful call.  rt_set_instance_types re-issues the records from the library's copy; frame batches (rt_set_batch) take host
 * records only, and a later rt_set_batch or rt_set_instances replaces the device instances. */
int rt_set_instances_device(rt_ctx* ctx, const void* d_instances, int n, int update, void* hip_stream);

/* BLAS update (Vulkan: a BLAS built with ALLOW_UPDATE, rebuilt with mode = UPDATE, src = dst) for deforming meshes: skinning, cloth,
 * morph targets.  d_verts6 = the mesh's new vertices in the rt_upload_geometry layout (interleaved px py pz nx ny nz) in memory of
 * ctx's GPU, covering the mesh's vertex span: from its first_float, 6 x (largest index the mesh references + 1) floats, which
 * n_floats must equal.  Positions and normals are replaced; indices, triangle count and materials stay.  The call waits for the
 * frames of every slot of the scene (the vertex buffer and the BLAS are shared and not double-buffered), copies the vertices into
 * the scene's vertex buffer in stream order on hip_stream (NULL = the context's stream: the caller may overwrite its buffer as soon
 * as the call returns), refits the BLAS on the device (same topology, new boxes and quantisation) and returns after one small
 * readback (the new root box).  Every slot's TLAS is then stale: its next frame needs rt_set_instances, rt_set_instances_device or
 * rt_set_batch first (update = 1 is accepted), else RT_ERR_NOT_READY.  Frames and hit records equal those of a fresh
 * rt_upload_geometry + rt_build_blas + rt_set_instances over the same vertices.  A later relink keeps the refit; a later
 * rt_build_blas of the mesh builds over the refitted vertices; rt_upload_geometry drops it.
 * RT_ERR_INVALID_ARGUMENT: a NULL pointer, a mesh index out of range, a wrong n_floats, a mesh without triangles or whose vertex
 * span overlaps another mesh's, trace_variant != 0, or a position that is not finite (the vertices are replaced by then: the mesh
 * counts as not built until a refit with finite positions or rt_build_blas); RT_ERR_NOT_READY: the mesh has no built BLAS, or a
 * frame of the scene submitted with rt_trace_async is pending. */
int rt_refit_blas_device(rt_ctx* ctx, int mesh, const void* d_verts6, size_t n_floats, void* hip_stream);

/* ---- MTL materials and a per-instance type table -------------------------------------------------
 * The reference's loader parses Kd/Ks/Ns/Ni/illum (include/tiny_obj_loader.h:565 GetMaterials) and its renderer ignores
 * them: src/shader.rgen:51-55 hard-codes ka (.1,.3,.1), kd (.2,1,.2), ks .8, exponent 100, index of refraction 1.52, and
 * src/shader.rgen:96 knows two object types ("Hardcoded as 2 objects", src/main.cpp:2425).  Both calls are optional:
 * without them every frame is the reference's, bit for bit. */
typedef struct rt_material {
  float ka[3]; float ns;        /* Ka;  Ns = specular exponent, applied as an integer power (rounded, 0..1023) */
  float kd[3]; float ni;        /* Kd;  Ni = index of refraction of a refractive surface */
  float ks[3]; uint32_t type;   /* Ks;  0 diffuse, 1 mirror, 2 refractive, or RT_MATERIAL_TYPE_OF_INSTANCE */
} rt_material;
#define RT_MATERIAL_TYPE_OF_INSTANCE 0xFFFFFFFFu   /* the surface's type is its instance's (rt_set_instance_types / the uniform block) */
/* table[prim_material[g]] shades triangle g of the shared index buffer, g = first_index / 3 + gl_PrimitiveID (one entry per
 * triangle: n_prims = n_idx / 3).  Scene state, shared by all frame slots; n_materials == 0 removes the table, and so does
 * rt_upload_geometry on any slot of the scene (the ids belong to the index buffer it replaces): frames are then shaded without a table
 * until it is set again with one id per triangle of the new index buffer (any other n_prims: RT_ERR_INVALID_ARGUMENT).  With a table the
 * diffuse branch evaluates Iamb*ka, kd, ks, pow(., Ns) and the refractive branch Ni from the hit triangle's material. */
int rt_set_materials(rt_ctx* ctx, const rt_material* table, int n_materials, const uint32_t* prim_material, size_t n_prims);
/* types[i] in {0,1,2} for instance i of this context's next rt_set_instances (and of the current ones, re-issued at once);
 * n == 0 restores `objectIndex == 0 ? centerObjectType : orbitingObjectType` (src/shader.rgen:96). */
int rt_set_instance_types(rt_ctx* ctx, const uint32_t* types, int n);

/* Uniform buffer copyData (src/main.cpp:1887-1889, 2901-2903).  RT_ERR_NOT_READY, with nothing changed, while the context holds a frame
 * batch (rt_set_batch with more than one frame): call rt_set_instances first.  The block is taken as it is; the calls that use it check
 * it: a frame call or rt_shade_rays_device with samplesPerPixel 0 (frames) or maxBounceCount above 69 returns RT_ERR_INVALID_ARGUMENT,
 * enqueues nothing and leaves a frame submitted before it, pending or not, as it was. */
int rt_set_uniforms(rt_ctx* ctx, const rt_uniforms* u);

/* Cube map creation + upload (src/main.cpp:2073-2412): 6 RGBA8 faces in the order
 * right,left,top,bottom,front,back (:2064-2071) = +X,-X,+Y,-Y,+Z,-Z, all w x h. */
int rt_set_skybox(rt_ctx* ctx, const uint8_t* const faces_rgba8[6], int w, int h);

/* vkCmdTraceRaysKHR(W,H,1) + the image copy (src/main.cpp:2620-2624, 2683-2686).  Blocking; writes the
 * whole frame (row 0 = top, RGBA32F, the shader's declared rgba32f format src/shader.rgen:48) to host. */
int rt_trace(rt_ctx* ctx, int width, int height, float* out_rgba32f_host, rt_stats* stats);

/* Sharded, asynchronous form used for multi-GPU tiling (one process per GPU).  d_out must stay valid, and is only guaranteed
 * complete, after the rt_synchronize / rt_get_stats that follows the call: should a grid barrier of the bounce kernel give
 * up (rt_stats.tail_faults), that call renders the frame again into d_out — from the uniforms and instance records the
 * frame was submitted with — and reports rt_stats.frames_rerendered = 1; work the caller enqueued behind the frame on its
 * own stream (a gather, a copy) has then consumed the incomplete frame and must be repeated.  Frames enqueued back to back
 * on one context without collecting each: a fault in an earlier one is still reported and switches the context to
 * per-bounce launches, but only the most recent frame is rendered again.  Renders the row bands
 * {b : b % n_shards == shard} of band_rows rows each and writes them COMPACTLY (band after band, each
 * band_rows x width x 4 floats; the last band of the frame may be short) into d_out, a DEVICE pointer
 * owned by the caller (e.g. a torch tensor), enqueued on hip_stream (NULL = the context's stream).
 * Returns immediately; use rt_synchronize / the stream to wait.  out_capacity_bytes guards d_out. */
int rt_trace_shard(rt_ctx* ctx, int width, int height, int band_rows, int shard, int n_shards,
                   void* d_out, size_t out_capacity_bytes, void* hip_stream);
/* Frame batches: K <= 8 CONSECUTIVE frames through ONE pass of the pipeline.  A rank of an N-GPU split renders only its bands, and a
 * 1/8 shard of one frame is eight kernel launches at their latency floors (measured: 0.084 ms per shard frame against 0.058 = 1/8 of a
 * whole frame) — the bands of K frames together are launches of whole-frame size again, and the N-GPU host makes one gather per batch.
 * This is the multi-GPU form of the reference's frames in flight (swapchain images, src/main.cpp:1203, 2905-2967): the frames of a batch
 * are rendered together and complete together.
 * rt_set_batch replaces rt_set_instances + rt_set_uniforms for the K frames: instances = n_frames x n records (frame k's at
 * instances + k * n, each frame a createTLAS(update) of the same topology, src/main.cpp:2848-2861), uniforms = n_frames blocks — the camera
 * (position, right, up, forward), the light's position and its intensity may differ from frame to frame; maxBounceCount, samplesPerPixel and
 * the two object types are the batch's: a block that differs from block 0 in one of them is refused (RT_ERR_INVALID_ARGUMENT, the context
 * keeps its state); the two informational offset fields are not compared.  update as in rt_set_instances.  Void, non-invertible and far
 * records as in rt_set_instances: the frames share ONE quantisation, and a void record of one frame adds nothing to it, so it changes no
 * other frame either.
 * While the context holds a batch of more than one frame its uniforms are the batch's: rt_set_uniforms returns RT_ERR_NOT_READY and changes
 * nothing; rt_set_instances (back to single frames) comes first, then rt_set_uniforms.  The frames of a batch are walked by the one-lane
 * kernels whatever "packet_trace" says.
 * rt_trace_shard_batch is rt_trace_shard for the batch: frame k's compact shard lands frame_stride_bytes behind frame k - 1's (0: back to
 * back, rows * width pixels apart); statistics are sums over the batch.  Results are those of the K frames rendered one by one, bit for bit (tested). */
int rt_set_batch(rt_ctx* ctx, int n_frames, const rt_instance* instances, int n, const rt_uniforms* uniforms, int update);
int rt_trace_shard_batch(rt_ctx* ctx, int width, int height, int band_rows, int shard, int n_shards,
                         void* d_out, size_t frame_stride_bytes, size_t out_capacity_bytes, void* hip_stream);
/* Frames in flight from a plain C/C++ host: rt_trace_async enqueues the frame and its copy to a pinned host buffer owned
 * by the context and returns (vkQueueSubmit with a fence, src/main.cpp:2905-2967); rt_trace_wait blocks until that frame
 * is complete (vkWaitForFences, src/main.cpp:772-778) and hands out the pixels (W*H*4 floats, or W*H*4 bytes with
 * rt_set_param "output_rgba8" 1; valid until the next rt_trace_async on this context) and the frame's counters.  One frame per context may be pending; a host that wants P
 * frames in flight keeps P contexts, as the reference keeps one command buffer, fence and image per swapchain image. */
int rt_trace_async(rt_ctx* ctx, int width, int height);
int rt_trace_wait(rt_ctx* ctx, const void** pixels, rt_stats* stats);

/* Root-side step of a multi-GPU frame (the analogue of the reference's vkCmdCopyImage into the presented image,
 * src/main.cpp:2683-2686): after the gather, n_shards compact shards (as rt_trace_shard writes them, shard s at byte
 * s * shard_stride_bytes) lie in d_gathered; this de-interleaves them into the width x height frame at d_frame (device
 * pointers of ctx's GPU; pixel format = ctx's, RGBA32F or RGBA8), enqueued on hip_stream (NULL = the context's). */
int rt_assemble_shards(rt_ctx* ctx, const void* d_gathered, int n_shards, size_t shard_stride_bytes, int width, int height,
                       int band_rows, void* d_frame, size_t frame_capacity_bytes, void* hip_stream);

/* number of rows rt_trace_shard writes for (height, band_rows, shard, n_shards) */
int rt_shard_rows(int height, int band_rows, int shard, int n_shards);

/* Wait for the last enqueued frame and read its counters / HIP-event timings. */
int rt_synchronize(rt_ctx* ctx);
int rt_get_stats(rt_ctx* ctx, rt_stats* stats);
/* Per-kernel hipEvent timing (default off): 1 = events around every kernel of a frame (each record between two kernels costs
 * ~10 us of idle GPU), 2 = around the closest-hit traversal launches only (rt_stats.ms_trace_closest; the other times read 0). */
int rt_set_timing(rt_ctx* ctx, int enabled);

/* Tunables (no reference counterpart): "trace_variant" 0 = quantized BVH2 / one lane per ray (default), 1 = BVH4 /
 * four lanes per ray, 2 = 4-ary records / one lane per ray; "tail_kernel" 0 = one launch per bounce and kernel, 1 = bounces
 * 1..maxBounceCount in one launch when the previous frame had few secondary rays (default), 2 = always;
 * "output_rgba8" 1 = every entry point that returns a frame stores 8-bit RGBA (clamp to [0,1], x255, round; the format
 * the reference's storage image really has, src/main.cpp:1899) instead of RGBA32F — a quarter of the PCIe bytes;
 * "trace_blocks_per_cu" 1..8; "shade_blocks_per_cu" 1..16; "blas_builder" 1 = device builder (default:
 * rt_build_blas builds on the GPU, as the reference's DEVICE build type does, src/main.cpp:345-357 — a binned-SAH tree made level by
 * level; the environment variable RT_GPU_BVH_ALGO = 1 / 2 selects the LBVH / PLOC builders instead), 0 = host binned-SAH (threaded);
 * "trace_rays_per_lane", "trace_min_blocks" size the persistent grids; "closest_blocks_per_cu" / "shadow_blocks_per_cu" cap one launch's share of
 * it (-1 = automatic, the default: 2 per CU for launches of at most 2.5 M rays when three or more frame slots share the GPU, 0 = no cap, 1..8); "primary_cover" 1 (default) = before ray generation the
 * frontier boxes of every instance's BLAS are projected onto 8x8-pixel screen tiles and the samples of tiles no mesh can
 * project onto are shaded as misses without any box test, 0 = every primary ray is tested against the TLAS;
 * "entry_points" 1 (default; needs primary_cover) = every marked tile gets an entry record — the handful of deep subtrees of the
 * TLAS / the nearest instance's BLAS that the tile's beam of primary rays can touch — and its primary rays start their walk there
 * instead of at the TLAS root; "shadow_entry" = the same for the shadow rays, from the tiles of a cube of "light_tiles" (8..512,
 * default 256) tiles per side around the light: 0 = off, 1 = rebuilt in every frame (measured: costs more than it saves), 2 (default) =
 * built once the light and the instances have stood still for two frames and kept until either moves (they do not depend on the camera); "packet_trace" 1 = primary and shadow rays are
 * walked by the packet kernel (one wavefront per 64-ray chunk; default 0: measured slower), 2 = rt_intersect's rays too;
 * "output_bgra8" 1 = like "output_rgba8" in the byte order of a B8G8R8A8 surface (surfaceFormatList[0] is normally that,
 * src/main.cpp:1204, 1899), so that a frame can be compared byte for byte with a screenshot of the original's swapchain image;
 * round 4: "pixel_beams" 1 (default) = the primary rays of a pixel share one walk (k_beam: boxes against the beam of the pixel's samples, triangles
 * per ray; frames without far rays), 0 = one walk per ray; "camera_records" 0 = no entry records for the primary rays (the light-side records stay);
 * "dead_shadow_rays" 1 (default) = a shadow ray whose outcome cannot change its sample (diffuse and specular exactly 0: the same bits lit or
 * shadowed) is settled when it is made and not walked — it still counts in rt_stats::rays_shadow, rays_shadow_untraced says how many — 0 = every
 * shadow ray is walked; "shadow_beams" 1 = the shadow rays of the primary hits in beams as well (k_beam_shadow; default 0: measured slower;
 * librt_mi355x_alt.so only — the product library refuses 1 with RT_ERR_INVALID_ARGUMENT);
 * "jitter_table" 1 (default) = k_raygen reads the sample positions of a frame size from a table made once, 0 = evaluates the hash per sample and frame;
 * "tile_blobs" 1 = the nodes and triangle packets of a screen tile staged through LDS (k_blob / k_tile; default 0: measured slower;
 * librt_mi355x_alt.so only, like "shadow_beams").  In the product library the tile-blob fields of rt_stats are always 0.
 * round 6: "fused_shade" 1 (default) = bounce 0 of a single frame with pixel beams is ONE launch: the kernel that walks a pixel's primary rays shades
 * their hits (k_beam_shade; not in counting frames, frame batches or with "camera_records" 0), 0 = the walk and the shading are two launches with the
 * hit records between them.  With timing on, rt_stats::ms_trace_closest of a fused frame covers walk + shading of bounce 0 and ms_shade the later bounces only.
 * Results do not depend on any of them. */
int rt_set_param(rt_ctx* ctx, const char* name, int value);

/* Record-level entry for traceRayEXT alone (rows a10/a14): n rays of 8 floats (o.xyz, tmin, d.xyz, tmax)
 * from host memory; any_hit!=0 = TerminateOnFirstHit|SkipClosestHit (src/shader.rgen:67). Blocking.
 * counting!=0 runs the instrumented kernel and fills stats->node_visits / tri_tests. */
int rt_intersect(rt_ctx* ctx, size_t n, const float* rays8_host, int any_hit, rt_hit* out_host, int counting,
                 rt_stats* stats);

/* Surface of a closest hit: what src/shader.rchit:50-96 computes before it shades (32 B, 16-B aligned in rt_intersect_device's output). */
typedef struct rt_hit_attr {
  float position[3];    /* P = o2w * (barycentric interpolation of the triangle's three positions) */
  int32_t object_index; /* gl_InstanceCustomIndexEXT; -1 on a miss */
  float normal[3];      /* N = normalize(interpolated normal * w2o), as the closest-hit shading takes it */
  uint32_t reserved;    /* 0 */
} rt_hit_attr;

/* Ray queries in device memory (VK_KHR_ray_query: rayQueryEXT from any shader), ordered on hip_stream (NULL = the context's stream).
 * d_rays8 = n rays in rt_intersect's layout (o.xyz, tmin, d.xyz, tmax: 32 B each, 16-B aligned); d_hits receives n rt_hit (4-B
 * aligned); d_attr, optional and for closest-hit queries only, n rt_hit_attr (16-B aligned; a miss gives zeros and object_index -1).
 * All three are memory of ctx's GPU.  Hits equal rt_intersect's bit for bit for both any_hit values.  Fully asynchronous: the rays are
 * read and the results written in stream order; no host copy, no host synchronisation, no wait for a frame in flight (a query has its
 * own counter block and spill area, allocated at the first query).  A query sees the TLAS of the last rt_set_instances* call before it
 * and the scene as it was at the call: later calls that rewrite that TLAS parity or the shared scene wait for it, rt_destroy too.  Queries
 * of one context from different streams run one after the other (stream waits, not host waits).  n == 0 enqueues nothing.  The quantised
 * BVH2 is always walked (packet_trace does not apply).
 * RT_ERR_INVALID_ARGUMENT: a NULL or misaligned pointer, a pointer that is not memory of ctx's GPU, n >= 0xFFFFFF00, d_attr with
 * any_hit != 0 (Vulkan's any hit here is SkipClosestHit), trace_variant != 0; RT_ERR_NOT_READY: as for a frame (no geometry, no TLAS,
 * a TLAS stale after rt_refit_blas_device, a frame batch held by the context). */
int rt_intersect_device(rt_ctx* ctx, size_t n, const void* d_rays8, int any_hit, void* d_hits, void* d_attr, void* hip_stream);

/* Ray flags and cull masks per query (rayQueryInitializeEXT(rq, tlas, rayFlags, cullMask, origin, tMin, direction, tMax)).  The values
 * are those of gl_RayFlags*EXT / SPIR-V RayFlags; the reference traces with Opaque (primary rays) and Opaque | TerminateOnFirstHit |
 * SkipClosestHit = 13 (shadow rays), cull mask 0xFF (src/shader.rgen:66-67). */
#define RT_RAY_FLAG_OPAQUE                 0x001u
#define RT_RAY_FLAG_NO_OPAQUE              0x002u
#define RT_RAY_FLAG_TERMINATE_ON_FIRST_HIT 0x004u
#define RT_RAY_FLAG_SKIP_CLOSEST_HIT       0x008u   /* no effect on a query */
#define RT_RAY_FLAG_CULL_BACK_FACING       0x010u
#define RT_RAY_FLAG_CULL_FRONT_FACING      0x020u
#define RT_RAY_FLAG_CULL_OPAQUE            0x040u
#define RT_RAY_FLAG_CULL_NO_OPAQUE         0x080u
#define RT_RAY_FLAG_SKIP_TRIANGLES         0x100u
#define RT_RAY_FLAG_SKIP_AABBS             0x200u   /* no effect: there are no AABB geometries */
/* VkGeometryInstanceFlagBitsKHR, in the high byte of rt_instance::sbt_offset_and_flags */
#define RT_INSTANCE_FLAG_FACING_CULL_DISABLE 0x1u
#define RT_INSTANCE_FLAG_FLIP_FACING         0x2u
#define RT_INSTANCE_FLAG_FORCE_OPAQUE        0x4u
#define RT_INSTANCE_FLAG_FORCE_NO_OPAQUE     0x8u
/* hit kinds in rt_hit_attr::reserved (gl_HitKindFrontFacingTriangleEXT / BackFacing), 0 on a miss */
#define RT_HIT_KIND_FRONT_FACING 0xFEu
#define RT_HIT_KIND_BACK_FACING  0xFFu

/* rt_intersect_device with per-ray flags and cull masks.  Rays, hits, attributes, stream, ordering, workspace and RT_ERR_NOT_READY are
 * those of rt_intersect_device.  d_ray_words, optional, is n uint32 in device memory of ctx's GPU (4-B aligned), read in stream order
 * like the rays: bits 0-9 are ray flags, bits 24-31 the ray's cull mask, bits 10-23 are ignored.  Ray i traces with
 * flags = ray_flags | (word & 0x3FF) and cull mask = cull_mask & (word >> 24); a NULL array acts as words of 0xFF000000.
 *  - cull mask: an instance with (mask & cull) == 0 is not entered;
 *  - opacity: every geometry is opaque (the reference builds them with VK_GEOMETRY_OPAQUE_BIT_KHR, src/main.cpp:330).  The ray's
 *    OPAQUE / NO_OPAQUE decides first (OPAQUE if a word sets both), then the instance's FORCE_OPAQUE / FORCE_NO_OPAQUE (FORCE_OPAQUE
 *    first).  SKIP_TRIANGLES, CULL_OPAQUE on opaque and CULL_NO_OPAQUE on non-opaque triangles skip the instance.  There is no
 *    candidate / confirm loop: a non-opaque triangle is committed as if the caller confirmed every candidate (rt_intersect_device_hits
 *    returns every candidate);
 *  - facing, decided in object space (an instance transform, mirroring included, does not change it): a triangle is FRONT-FACING when
 *    det = dot(e1, cross(d, e2)) < 0 (e1 = v1 - v0, e2 = v2 - v0, d the object-space direction), i.e. its vertices appear clockwise
 *    from the ray origin in a right-handed object space (the DXR / VK_NV_ray_tracing default; VK_KHR's FLIP_FACING is aliased
 *    TRIANGLE_FRONT_COUNTERCLOCKWISE).  FLIP_FACING inverts it.  CULL_BACK_FACING / CULL_FRONT_FACING reject triangles before they can be
 *    accepted, unless the instance has FACING_CULL_DISABLE (rt_host.hpp's make_instance sets it on every instance, as the reference);
 *  - TERMINATE_ON_FIRST_HIT: the ray stops at its first accepted hit (rt_intersect_device's any_hit = 1); closest-hit and first-hit
 *    rays may be mixed in one call.
 * d_attr (optional, also for first-hit rays) receives rt_intersect_device's P, N and objectIndex, and the hit kind in `reserved`
 * (RT_HIT_KIND_*, 0 on a miss).
 * RT_ERR_INVALID_ARGUMENT: as for rt_intersect_device, and d_ray_words misaligned or not memory of ctx's GPU; ray_flags with bits
 * outside 0x3FF, cull_mask > 0xFF, more than one of OPAQUE, NO_OPAQUE, CULL_OPAQUE and CULL_NO_OPAQUE, both facing culls, or
 * SKIP_TRIANGLES with SKIP_AABBS or a facing cull (Vulkan's valid-usage rules).  Per-ray words are not validated (that would need a
 * host round trip): they follow the formulas above as written. */
int rt_intersect_device_flags(rt_ctx* ctx, size_t n, const void* d_rays8, const void* d_ray_words, uint32_t ray_flags, uint32_t cull_mask, void* d_hits, void* d_attr, void* hip_stream);

/* All hits along a ray: rayQueryProceedEXT's candidate loop in data form (every candidate, in order, and how many there are), for
 * inside/outside parity, multi-return LiDAR, depth peeling and thickness.  Rays, words, ray_flags and cull_mask as for
 * rt_intersect_device_flags.  The candidates C(ray) are every (inst, prim) that rt_intersect_device_flags may accept for the ray under the
 * same rules: the ray's [tmin, tmax], the flags and cull mask of the call and of the ray's word, instance masks, opacity with FORCE_*,
 * facing culls with FLIP_FACING and FACING_CULL_DISABLE, SKIP_TRIANGLES.  Every candidate is accepted: there is no caller code in the loop.
 *  - order: by (t, inst, prim) ascending, the closest-hit tie rule, so entry 0 is rt_intersect_device_flags' closest hit
 *    byte for byte; an (inst, prim) appears at most once;
 *  - d_hits: n x max_hits rt_hit, ray-major (hit j of ray i at i * max_hits + j); the entries past min(|C|, max_hits) are rt_intersect's
 *    miss (t = tmax, u = v = 0, prim = inst = -1);
 *  - d_attr (optional): n x max_hits rt_hit_attr in the same order, P, N, objectIndex and the hit kind in `reserved`, as
 *    rt_intersect_device_flags fills them; a miss is zeros, object_index -1, kind 0;
 *  - d_counts (optional): n uint32, |C(ray)| over the whole interval, not capped at max_hits.  Without it the walk may stop looking
 *    beyond the max_hits-th entry; the lists are the same either way;
 *  - max_hits 1..16, or 0 = count only: then d_hits and d_attr must be NULL and d_counts non-NULL.
 * TERMINATE_ON_FIRST_HIT in ray_flags is RT_ERR_INVALID_ARGUMENT (a multi-hit query has no first-hit form); in a ray's word the bit is
 * ignored.  SKIP_CLOSEST_HIT and SKIP_AABBS have no effect.  Parity: the canonical triangle test is not watertight, so a ray through a
 * shared edge or vertex may be counted by both triangles or by neither; |C| % 2 is exact only for rays that pass away from edges.
 * Alignment (rays and attributes 16 B; ray words, hits and counts 4 B), device memory of ctx's GPU, stream ordering without host
 * synchronisation, the TLAS and scene of the call, queries of one context one after another, RT_ERR_NOT_READY and n == 0: as for
 * rt_intersect_device_flags.  The query's workspace is rt_intersect_device's.
 * RT_ERR_INVALID_ARGUMENT: as for rt_intersect_device_flags; max_hits > 16; max_hits == 0 with d_hits or d_attr or without d_counts;
 * n >= 0xFFFFFF00, or n x max_hits >= 0xFFFFFF00 (the kernels index records with 32 bits). */
int rt_intersect_device_hits(rt_ctx* ctx, size_t n, const void* d_rays8, const void* d_ray_words, uint32_t ray_flags, uint32_t cull_mask,
                             uint32_t max_hits, void* d_hits, void* d_attr, void* d_counts, void* hip_stream);

/* Closest points: for every query point the nearest point of the scene's surface (Embree's point queries, Open3D's
 * compute_closest_points), for distance fields, collision and penetration depth, snapping samples to a surface and nearest-surface
 * attributes of point clouds.  The one query of the family that is not a ray.
 * Points: d_points4 holds n records of 16 B (x, y, z, r_max), 16-B aligned, memory of ctx's GPU: a world-space point and a search
 * radius, r_max >= 0 (+inf allowed).
 * Candidates: every triangle of every instance with (mask & cull_mask) != 0.  Instance flags, opacity and facing play no part.
 * d_hits: n rt_hit, 4-B aligned.  Record i is the candidate with the smallest key (d2, inst, prim) among those with
 * d2 <= r_max * r_max (the product rounded to binary32), d2 the canonical squared distance below: t = sqrtf(d2) is the world-space
 * distance to the nearest point, u and v that point's barycentrics of vertices B and C (a hit's convention), prim and inst the triangle.
 * Nothing within r_max: the miss record t = r_max as given, u = v = 0, prim = inst = -1; the same for a non-finite coordinate, a negative
 * r_max or a NaN r_max.  t is never NaN unless r_max was.
 * Canonical arithmetic (DESIGN.md §5 "Closest points" has the full sequence): binary32, nothing fused except inside dot3 / xform_point /
 * xform_vec, which are the library's.  For instance I and triangle packet (v0, e1, e2): a = xform_point(I.o2w, v0),
 * ab = xform_vec(I.o2w, e1), ac = xform_vec(I.o2w, e2); the vertex / edge / face regions of Ericson, Real-Time Collision Detection
 * §5.1.5, over ap = p - a, d1..d6, vc, vb, va in that order with its <= / >= comparisons and IEEE divisions;
 * c = ap - (u * ab + v * ac), d2 = dot3(c, c).  d2 depends on the point, the instance record and the packet only, never on the tree; a
 * triangle whose d2 is NaN (zero-area triangles only) is never a candidate.
 * Needles (aspect 1e-4 and below) are answered with that same arithmetic, whose (u, v) is then rounding noise: the reported t can be
 * off by the length of the needle.
 * d_attr (optional): n rt_hit_attr, 16-B aligned: what rt_intersect_device gives for a hit with this (inst, prim, u, v) — P the nearest
 * point, N the interpolated shading normal, objectIndex; a miss zeros and -1.  `reserved` is the side of the triangle's plane the point
 * lies on: RT_HIT_KIND_FRONT_FACING when s = dot(cross(e1, e2), xform_point(I.w2o, p) - v0) < 0, else RT_HIT_KIND_BACK_FACING (e1, e2,
 * v0 from the vertex buffer), inverted by FLIP_FACING, 0 on a miss: the kind rt_intersect_device_flags reports for a ray from the point
 * that hits that triangle.  Like parity it is a per-triangle sign, not a robust inside/outside test near edges and vertices.
 * Stream ordering without host synchronisation, the TLAS and scene of the call, the query workspace, queries and shading calls of one
 * context one after another, RT_ERR_NOT_READY and n == 0 (nothing is enqueued): as for rt_intersect_device.
 * RT_ERR_INVALID_ARGUMENT: a NULL or misaligned pointer, a pointer that is not memory of ctx's GPU, n >= 0xFFFFFF00, cull_mask > 0xFF,
 * trace_variant != 0. */
int rt_closest_point_device(rt_ctx* ctx, size_t n, const void* d_points4, uint32_t cull_mask, void* d_hits, void* d_attr, void* hip_stream);
/* The blocking host form, as rt_intersect is to rt_intersect_device: the records are copied to the device, queried on the context's
 * stream (same workspace and ordering) and the results copied back.  counting != 0 runs the instrumented walk and fills
 * stats->node_visits and stats->tri_tests (boxes-pair visits and point-triangle tests of the whole call); stats may be NULL. */
int rt_closest_point(rt_ctx* ctx, size_t n, const float* points4_host, uint32_t cull_mask, rt_hit* out_host, int counting, rt_stats* stats);

/* The K nearest triangles of every query point and the number of triangles within its radius: rt_closest_point_device's list form, as
 * rt_intersect_device_hits is rt_intersect_device_flags'.  For contact manifolds (a sphere or particle against the scene needs every
 * triangle within its radius), PhysX's overlapSphere count, a stable normal / material / object id near vertices and edges (blend or
 * vote over the few nearest triangles) and k-nearest surface samples.
 * Points: rt_closest_point_device's records (x, y, z, r_max), 16-B aligned: one buffer feeds both calls.
 * Candidates C(p): every triangle of every instance with (mask & cull_mask) != 0 is tested; it is a candidate when its canonical d2
 * (rt_closest_point_device, DESIGN.md §5 "Closest points") is not NaN and d2 <= r_max * r_max (the product rounded to binary32).  This is
 * exactly the set rt_closest_point_device takes its minimum from: the bound is inclusive, and with r_max = +inf a d2 of +inf is a
 * candidate, as it is there.  Instance flags, opacity and facing play no part; void and non-invertible instance records behave as
 * they do for rt_closest_point_device.
 *  - d_hits: n x max_hits rt_hit, point-major (entry j of point i at i * max_hits + j), 4-B aligned.  A row holds the max_hits smallest
 *    candidates by the key (d2, inst, prim) ascending.  The order is d2's, not t's: two different d2 can round to the same sqrtf, and
 *    then (inst, prim) must not reorder them.  In each entry t = sqrtf(d2), u and v the nearest point's barycentrics of B and C.  Entry 0
 *    is rt_closest_point_device's record byte for byte; an (inst, prim) appears at most once.  Entries past min(|C|, max_hits) are the
 *    miss form: t = r_max as given (bit pattern kept), u = v = 0, prim = inst = -1;
 *  - d_counts (optional): n uint32, 4-B aligned: |C(p)|, not capped at max_hits.  Without it the walk may stop looking beyond the
 *    max_hits-th entry's d2 once the row is full; the rows are the same either way.  With it and r_max = +inf the walk visits every
 *    admitted triangle of the scene: that is the caller's choice;
 *  - max_hits 1..16, or 0 = count only: then d_hits and d_attr must be NULL and d_counts non-NULL.  That form is the sphere-overlap
 *    count.  Occupancy ("anything within r") is rt_closest_point_device's inst >= 0 and needs no flag here;
 *  - d_attr (optional): n x max_hits rt_hit_attr, 16-B aligned, in the same order: what rt_closest_point_device gives for that
 *    (inst, prim, u, v) and that point: P, N, objectIndex and the side word in `reserved`; a miss is zeros, -1 and 0.
 * Invalid records (a non-finite coordinate, a negative or NaN r_max): a row of miss forms and a count of 0.
 * Stream ordering without host synchronisation, the TLAS and scene of the call, the query workspace, queries and shading calls of one
 * context one after another, RT_ERR_NOT_READY and n == 0 (nothing is enqueued): as for rt_closest_point_device.
 * RT_ERR_INVALID_ARGUMENT: a NULL or misaligned pointer, a pointer that is not memory of ctx's GPU, n >= 0xFFFFFF00 or
 * n x max_hits >= 0xFFFFFF00 (the kernels index records with 32 bits), cull_mask > 0xFF, max_hits > 16, max_hits == 0 with d_hits or
 * d_attr or without d_counts, trace_variant != 0. */
int rt_closest_point_device_hits(rt_ctx* ctx, size_t n, const void* d_points4, uint32_t cull_mask, uint32_t max_hits,
                                 void* d_hits, void* d_attr, void* d_counts, void* hip_stream);
/* The blocking host form, as rt_closest_point is to rt_closest_point_device: the records are copied to the device, queried on the
 * context's stream (same workspace and ordering) and hits_host (n x max_hits records; NULL with max_hits 0) and counts_host (n; optional
 * unless max_hits is 0) copied back.  counting != 0 runs the instrumented walk and fills stats->node_visits and stats->tri_tests; stats
 * may be NULL.  As rt_closest_point does, the call also reports the walk's device time in stats->ms_trace_closest and the node and
 * packet sizes in stats->bvh_node_bytes / bvh_tri_bytes; every other field is 0. */
int rt_closest_point_hits(rt_ctx* ctx, size_t n, const float* points4_host, uint32_t cull_mask, uint32_t max_hits,
                          rt_hit* hits_host, uint32_t* counts_host, int counting, rt_stats* stats);

/* Box overlaps: for every query box the triangles of the scene that touch it (PhysX's overlap query, an occupancy test per voxel), for
 * voxelisation and occupancy grids, broad-phase collision against the live scene, region selection and "is this cell empty" tests.
 * Boxes: d_boxes8 holds n records of 32 B (lo.x, lo.y, lo.z, w3, hi.x, hi.y, hi.z, w7), 16-B aligned, memory of ctx's GPU: a closed
 * world-space axis-aligned box; words 3 and 7 are ignored.  lo == hi on any axis is allowed (a plane, a line, a point).  A record with a
 * non-finite bound or with lo > hi on an axis is invalid: its count is 0 and it lists nothing.
 * Candidates C(box): the triangles of every instance with (mask & cull_mask) != 0 that the canonical predicate below does not separate
 * from the box.  Both sets are closed: touching counts.  Instance flags, opacity and facing play no part.
 * d_counts (optional): n uint32, 4-B aligned: |C(box)|, not capped at max_ids.
 * d_ids: n x max_ids records of 8 B (int32 inst, int32 prim), 4-B aligned, box-major: a row lists the max_ids smallest candidates by
 * (inst, prim) ascending, entries past min(|C|, max_ids) are (-1, -1).  max_ids is 0..16; with 0 the call counts only (d_ids NULL,
 * d_counts non-NULL).  Without d_counts the walk stops looking for ids larger than a full row's last entry; the rows are the same.
 * RT_OVERLAP_ANY in flags answers occupancy: max_ids must be 0, d_counts receives 0 or 1 (|C| > 0) and the walk of a box ends at its
 * first candidate.
 * Canonical predicate (DESIGN.md §5 "Box overlaps" has every operation in order): binary32, nothing fused except inside dot3 / cross3 /
 * xform_point / xform_vec.  A = xform_point(I.o2w, v0), ab = xform_vec(I.o2w, e1), ac = xform_vec(I.o2w, e2), B = A + ab,
 * C = A + ac (a non-finite A, B or C: never a candidate); the box axes on lo / hi themselves; then with c = 0.5 lo + 0.5 hi,
 * h = 0.5 hi - 0.5 lo and the centred vertices the nine axes e_i x f_j and the triangle's plane of Akenine-Moller's "Fast 3D
 * Triangle-Box Overlap Testing".  Every comparison is strict: a tie is not a separation.  The predicate depends on the box, the instance
 * record and the packet only, never on the tree.
 * Stream ordering without host synchronisation, the TLAS and scene of the call, the query workspace, queries and shading calls of one
 * context one after another, RT_ERR_NOT_READY and n == 0 (nothing is enqueued): as for rt_closest_point_device.
 * RT_ERR_INVALID_ARGUMENT: a NULL or misaligned pointer, a pointer that is not memory of ctx's GPU, n >= 0xFFFFFF00 or
 * n x max_ids >= 0xFFFFFF00, cull_mask > 0xFF, unknown flag bits, max_ids > 16, max_ids == 0 with d_ids or without d_counts,
 * RT_OVERLAP_ANY with max_ids != 0, neither output given, trace_variant != 0. */
#define RT_OVERLAP_ANY 0x1u
int rt_overlap_boxes_device(rt_ctx* ctx, size_t n, const void* d_boxes8, uint32_t cull_mask, uint32_t flags,
                            uint32_t max_ids, void* d_ids, void* d_counts, void* hip_stream);
/* The blocking host form, as rt_closest_point is to rt_closest_point_device: the boxes are copied to the device, queried on the
 * context's stream (same workspace and ordering) and ids_host (n x max_ids pairs; NULL with max_ids 0) and counts_host (n; optional
 * unless max_ids is 0) copied back.  counting != 0 runs the instrumented walk and fills stats->node_visits and stats->tri_tests (node
 * visits and triangle-box tests of the whole call); stats may be NULL.  As rt_closest_point does, the call also reports the walk's device
 * time in stats->ms_trace_closest and the node and packet sizes in stats->bvh_node_bytes / bvh_tri_bytes; every other field is 0. */
int rt_overlap_boxes(rt_ctx* ctx, size_t n, const float* boxes8_host, uint32_t cull_mask, uint32_t flags,
                     uint32_t max_ids, int32_t* ids_host, uint32_t* counts_host, int counting, rt_stats* stats);

/* Triangle overlaps: for every query triangle the triangles of the scene that cut or touch it (Embree's rtcCollide, FCL's mesh collision
 * with the scene as one side), for cloth and tools whose vertices live in device memory, a robot link against its environment,
 * self-collision through the cull mask, and the first step of cutting and CSG.
 * Triangles: d_tris12 holds n records of 48 B (P0.x, P0.y, P0.z, w3, P1.x, P1.y, P1.z, w7, P2.x, P2.y, P2.z, w11), 16-B aligned, memory
 * of ctx's GPU: a closed world-space triangle; words 3, 7 and 11 are ignored.  A record with a non-finite vertex component is invalid:
 * its count is 0 and it lists nothing.  A zero-area query (a segment, a point) is valid and answered by the same arithmetic.
 * Candidates C(query): the triangles of every instance with (mask & cull_mask) != 0 that the canonical predicate below does not separate
 * from the query.  Both sets are closed: touching counts.  Instance flags, opacity and facing play no part.  Query triangles that are
 * triangles of the scene itself are better named by reference (rt_overlap_scene_triangles_device below), which leaves out their own
 * instance by rule; for query triangles that are not in the scene, cull_mask is how a caller leaves out an instance they came from.
 * d_counts, d_ids, max_ids, RT_OVERLAP_ANY in flags, the pruning without d_counts: exactly as for rt_overlap_boxes_device.
 * Canonical predicate (DESIGN.md §5 "Triangle overlaps" has every operation in order): binary32, nothing fused except inside dot3 /
 * cross3 / xform_point / xform_vec, min / max are fminf / fmaxf.  A, B, C as for rt_overlap_boxes_device (a non-finite A, B
 * or C: never a candidate); the bounds of A, B, C against the bounds of P0, P1, P2 on every axis; then, centred on P0 (p1 = P1 - P0,
 * p2 = P2 - P0, a = A - P0, b = B - P0, c = C - P0), with the edges g0 = p1, g1 = p2 - p1, g2 = p2 and f0 = b - a, f1 = c - b, f2 = a - c
 * and the normals n = cross3(g0, g2), m = cross3(f0, f1), seventeen axes L in this order: n, m, the nine cross3(g_i, f_j) i-major, the
 * three cross3(n, g_i), the three cross3(m, f_j).  On each the query projects to 0, dot3(L, p1), dot3(L, p2) and the candidate to
 * dot3(L, a), dot3(L, b), dot3(L, c); the pair is separated if the query's minimum is greater than the candidate's maximum or its maximum
 * less than the candidate's minimum.  Every comparison is strict: a tie is not a separation, and a zero axis separates nothing.  The
 * predicate depends on the query record, the instance record and the packet only, never on the tree.  One exception to "never on the
 * tree": a zero-area triangle has an incomplete axis set, and a pair of two zero-area triangles that nothing but their bounds holds
 * together (a point beside a segment, say) may be left out, because the walk need not come near it; a pair in which either triangle
 * has an area is always decided by the predicate.
 * Stream ordering, the TLAS and scene of the call, the workspace, RT_ERR_NOT_READY, n == 0 (nothing is enqueued) and the
 * RT_ERR_INVALID_ARGUMENT list: as for rt_overlap_boxes_device, with d_tris12 in the place of d_boxes8. */
int rt_overlap_triangles_device(rt_ctx* ctx, size_t n, const void* d_tris12, uint32_t cull_mask, uint32_t flags,
                                uint32_t max_ids, void* d_ids, void* d_counts, void* hip_stream);
/* The blocking host form, as rt_overlap_boxes is to rt_overlap_boxes_device: ids_host (n x max_ids pairs; NULL with max_ids 0) and
 * counts_host (n; optional unless max_ids is 0) are copied back.  counting != 0 runs the instrumented walk and fills stats->node_visits
 * and stats->tri_tests (node visits and triangle-triangle tests of the whole call; packets are counted before the test, so with counts
 * requested both equal rt_overlap_boxes' on the queries' bounding boxes); stats may be NULL.  The timing and size fields as for
 * rt_overlap_boxes. */
int rt_overlap_triangles(rt_ctx* ctx, size_t n, const float* tris12_host, uint32_t cull_mask, uint32_t flags,
                         uint32_t max_ids, int32_t* ids_host, uint32_t* counts_host, int counting, rt_stats* stats);

/* Sphere sweeps: for every record the first contact of a sphere that moves along a direction (PhysX's sweep query), for continuous
 * collision detection, character controllers, camera booms, clearance along a path and thick-beam sensors.
 * Sweeps: d_sweeps8 holds n records of 32 B (o.x, o.y, o.z, r, d.x, d.y, d.z, tmax), 16-B aligned, memory of ctx's GPU: a ray's layout
 * with the radius where tmin sits.  The sphere of radius r >= 0 has its centre at p(t) = o + t d for t in [0, tmax]; d need not be
 * normalised, t is in units of d, tmax = +inf is allowed.
 * Candidates: every triangle of every instance with (mask & cull_mask) != 0.  Instance flags, opacity and facing play no part.
 * d_hits: n rt_hit, 4-B aligned.  Record i is the candidate with the smallest key (t, inst, prim) among those whose canonical contact
 * time below exists and is <= tmax: t the first time the sphere touches the triangle, u and v the contact point's barycentrics of
 * vertices B and C (a hit's convention), prim and inst the triangle.  A sphere that touches a triangle at t = 0 already reports t = 0
 * with the closest-point barycentrics of o on that triangle.  No contact: the miss record t = tmax as given, u = v = 0,
 * prim = inst = -1; the same for a non-finite component of o, d or r, r < 0, d = 0, tmax < 0 or a NaN tmax.  t is never NaN unless tmax
 * was.
 * Canonical contact time (DESIGN.md §5 "Sphere sweeps" has every operation in order): binary32, world space, nothing fused except
 * inside dot3 / cross3 / xform_point / xform_vec.  A = xform_point(I.o2w, v0), ab = xform_vec(I.o2w, e1),
 * ac = xform_vec(I.o2w, e2) (non-finite: never a candidate); rt_closest_point_device's sequence for p = o decides the initial overlap
 * (d2 <= r * r: t = 0); otherwise the path is re-centred at its point nearest to A (t_c clamped to [0, tmax]) and the features of
 * Ericson, Real-Time Collision Detection §5.5.6 are tested from there: the face (plane contact, accepted when its barycentrics lie in
 * the triangle and the point they stand for is the contact point within 2^-10 of the longer edge, dot3(c, c) <= 2^-20 max(d00, d11):
 * a needle or zero-area triangle whose 2 x 2 system is rounding noise is answered by its edges and vertices), else the entering roots of the edge cylinders AB, AC, BC and the vertex spheres A, B, C, the smallest root in
 * [0, tmax], the earlier feature on a tie.  It depends on the record, the instance record and the packet only, never on the tree.
 * r = 0 is valid and answered by this arithmetic; bitwise equality with rt_intersect_device is not promised.  The edge and vertex
 * quadratics lose about 2^-24 (E + r)^2 / r of the radius for a triangle with longest edge E.
 * d_attr (optional): n rt_hit_attr, 16-B aligned: what rt_closest_point_device gives for (inst, prim, u, v) — P the contact point, N the
 * interpolated shading normal, objectIndex; a miss zeros and -1.  `reserved` is the side of the triangle's plane the centre
 * p(t) = o + t d lies on, by rt_closest_point_device's rule (FLIP_FACING included), 0 on a miss.  The contact normal is (p(t) - P) / r;
 * the caller forms it.
 * Stream ordering without host synchronisation, the TLAS and scene of the call, the query workspace, queries and shading calls of one
 * context one after another, RT_ERR_NOT_READY and n == 0 (nothing is enqueued): as for rt_closest_point_device.
 * RT_ERR_INVALID_ARGUMENT: a NULL or misaligned pointer, a pointer that is not memory of ctx's GPU, n >= 0xFFFFFF00, cull_mask > 0xFF,
 * trace_variant != 0. */
int rt_sweep_spheres_device(rt_ctx* ctx, size_t n, const void* d_sweeps8, uint32_t cull_mask,
                            void* d_hits, void* d_attr, void* hip_stream);
/* The blocking host form, as rt_closest_point is to rt_closest_point_device: the records are copied to the device, swept on the
 * context's stream (same workspace and ordering) and the hits copied back.  counting != 0 runs the instrumented walk and fills
 * stats->node_visits and stats->tri_tests; stats may be NULL.  As rt_overlap_boxes does, the call also reports the walk's device time in
 * stats->ms_trace_closest and the node and packet sizes in stats->bvh_node_bytes / bvh_tri_bytes; every other field is 0. */
int rt_sweep_spheres(rt_ctx* ctx, size_t n, const float* sweeps8_host, uint32_t cull_mask,
                     rt_hit* out_host, int counting, rt_stats* stats);

/* Closest points of segments: for every record the nearest pair of a point of a line segment and a point of the scene's surface
 * (PhysX's overlapCapsule and computePenetration, FCL's capsule distance): a capsule is a segment with a radius, so this is the
 * clearance of a robot link, the penetration depth and direction of a character's capsule, the nearest surface point of a cloth or
 * rope edge.
 * Records: d_segs8 holds n records of 32 B (P0.x, P0.y, P0.z, r_max, P1.x, P1.y, P1.z, w7), 16-B aligned, memory of ctx's GPU: the
 * closed world-space segment P0..P1 and the search radius r_max >= 0 (+inf allowed); word 7 is ignored.  P0 == P1 is valid (below).
 * Candidates: every triangle of every instance with (mask & cull_mask) != 0.  Instance flags, opacity and facing play no part; void and
 * non-invertible instance records behave as they do for rt_closest_point_device.
 * d_hits: n rt_hit, 4-B aligned.  Record i is the candidate with the smallest key (d2, inst, prim) among those whose canonical d2 below
 * is not NaN and is <= r_max * r_max (the product rounded to binary32; inclusive, as for closest points): t = sqrtf(d2), u and v the
 * barycentrics (of vertices B and C) of the triangle's point of the nearest pair, prim and inst the triangle.
 * d_params (optional): n floats, 4-B aligned: s in [0, 1], the segment's point of the nearest pair being P0 + s (P1 - P0); 0 on a miss.
 * No candidate: the miss record t = r_max as given (bit pattern kept), u = v = 0, prim = inst = -1, s = 0; the same for a non-finite
 * endpoint coordinate, a negative or a NaN r_max.  t is never NaN unless r_max was.
 * Canonical d2 (DESIGN.md §5 "Closest points of segments" has every operation in order): binary32, world space, nothing fused except
 * inside dot3 / cross3 / xform_point / xform_vec, IEEE divisions, clamp(x) = fminf(fmaxf(x, 0), 1) with NaN and -0 giving
 * +0.  a = xform_point(I.o2w, v0), ab = xform_vec(I.o2w, e1), ac = xform_vec(I.o2w, e2), d = P1 - P0.  Every feature proposes a pair of
 * a segment point and a triangle point and its d2 is the distance computed between the two, never an assumed 0: (1) rt_closest_point_device's
 * sequence for p = P0, s = 0; (2) the same for p = P1, s = 1; (3) only when the endpoints lie strictly on opposite sides of the
 * triangle's plane (h0 = dot3(n, P0 - a), h1 = dot3(n, P1 - a), n = cross3(ab, ac)): the same for the crossing X = P0 + s d,
 * s = clamp(h0 / (h0 - h1)); (4) the edges AB, AC, BC by Ericson, Real-Time Collision Detection §5.1.9 with exact-zero tests in place of
 * its epsilons.  A later feature replaces an earlier one only when its d2 is strictly smaller; a feature with a NaN d2 is skipped, a
 * triangle all of whose features are NaN is never a candidate.  The value depends on the record, the instance record and the packet
 * only, never on the tree.
 * Points: a record whose endpoints compare equal in all three components is answered by feature (1) alone: its rt_hit is
 * rt_closest_point_device's record for (P0, r_max) byte for byte, and s = 0.
 * Pierced triangles: a triangle the segment passes through reports the rounding residue of feature (3), a t around 2^-24 of the scene's
 * magnitude, not an exact 0: compare t with a radius or a tolerance.  Among several pierced triangles the key decides, not the order
 * along the segment; the first triangle along a segment is a ray query (rt_intersect_device).
 * d_attr (optional): n rt_hit_attr, 16-B aligned: what rt_closest_point_device gives for (inst, prim, u, v) — P the surface point, N the
 * interpolated shading normal, objectIndex; a miss zeros and -1.  `reserved` is the side of the triangle's plane the segment's point
 * P0 + s d lies on (per component one product and one sum), by rt_closest_point_device's rule (FLIP_FACING included), 0 on a miss.
 * Stream ordering without host synchronisation, the TLAS and scene of the call, the query workspace, queries and shading calls of one
 * context one after another, RT_ERR_NOT_READY and n == 0 (nothing is enqueued): as for rt_closest_point_device.
 * RT_ERR_INVALID_ARGUMENT: a NULL pointer (d_attr and d_params aside), a misaligned pointer, a pointer that is not memory of ctx's GPU,
 * n >= 0xFFFFFF00, cull_mask > 0xFF, trace_variant != 0. */
int rt_closest_segment_device(rt_ctx* ctx, size_t n, const void* d_segs8, uint32_t cull_mask,
                              void* d_hits, void* d_attr, void* d_params, void* hip_stream);
/* The blocking host form, as rt_closest_point is to rt_closest_point_device: the records are copied to the device, walked on the
 * context's stream (same workspace and ordering) and the hits and, with params_host, the parameters copied back.  counting != 0 runs
 * the instrumented walk and fills stats->node_visits and stats->tri_tests; stats may be NULL.  As rt_closest_point does, the call also
 * reports the walk's device time in stats->ms_trace_closest and the node and packet sizes in stats->bvh_node_bytes / bvh_tri_bytes;
 * every other field is 0. */
int rt_closest_segment(rt_ctx* ctx, size_t n, const float* segs8_host, uint32_t cull_mask,
                       rt_hit* out_host, float* params_host, int counting, rt_stats* stats);

/* Closest points of triangles: for every record the nearest pair of a point of a query triangle and a point of the scene's surface
 * (FCL's distance beside collide, PQP's TriDist, the mesh-mesh closest points of Bullet and PhysX): the distance half of
 * rt_overlap_triangles_device, for geometry that lives in device memory: the clearance of a tool or link mesh, cloth-to-body proximity
 * per face (its vertex-face and edge-edge pairs alike), the minimum separation of a whole mesh as the minimum over its records.
 * Records: d_tris12 holds n records of 48 B (P0.xyz, w3, P1.xyz, w7, P2.xyz, w11), 16-B aligned, memory of ctx's GPU:
 * rt_overlap_triangles_device's record, a closed world-space triangle.  Word 3 is the search radius r_max >= 0 (+inf allowed); words 7
 * and 11 are ignored.  One buffer feeds both triangle queries: the overlap query ignores word 3.  Degenerate triangles (a segment, a
 * point) are valid (below).
 * Candidates: every triangle of every instance with (mask & cull_mask) != 0.  Instance flags, opacity and facing play no part; void and
 * non-invertible instance records behave as they do for rt_closest_point_device.
 * d_hits: n rt_hit, 4-B aligned.  Record i is the candidate with the smallest key (d2, inst, prim) among those whose canonical d2 below
 * is not NaN and is <= r_max * r_max (the product rounded to binary32; inclusive, as for closest points): t = sqrtf(d2), u and v the
 * barycentrics (of vertices B and C) of the scene triangle's point of the nearest pair, prim and inst the scene triangle.
 * d_params (optional): n x 2 floats, 4-B aligned: (qu, qv), the barycentrics of the query's point of the nearest pair, which is
 * P0 + qu (P1 - P0) + qv (P2 - P0); both are in [0, 1] and never carry a sign bit; 0, 0 on a miss.
 * No candidate: the miss record t = r_max as given (bit pattern kept), u = v = 0, prim = inst = -1, qu = qv = 0; the same for a
 * non-finite vertex coordinate, a negative or a NaN r_max.  t is never NaN unless r_max was.
 * Canonical d2 (DESIGN.md §5 "Closest points of triangles" has every operation in order): binary32, world space, nothing fused except
 * inside dot3 / cross3 / xform_point / xform_vec, IEEE divisions, clamp as for rt_closest_segment_device.
 * a = xform_point(I.o2w, v0), ab = xform_vec(I.o2w, e1), ac = xform_vec(I.o2w, e2), b = a + ab, c = a + ac; g0 = P1 - P0, g2 = P2 - P0.
 * Every feature proposes a pair of a query point and a scene point and its d2 is the distance computed between the two, never an assumed
 * 0.  In this order: (1) rt_closest_point_device's sequence for p = P0, P1, P2, (qu, qv) = (0, 0), (1, 0), (0, 1); (2) for the query's
 * edges (P0, P1), (P1, P2), (P2, P0), feature (3) of rt_closest_segment_device (only when the ends lie strictly on opposite sides of
 * the scene triangle's plane: the same sequence for the crossing X = Pi + s (Pj - Pi)), (qu, qv) = (s, 0), (1 - s, s), (0, 1 - s);
 * (3) for each of those edges in turn, feature (4) of rt_closest_segment_device against AB, AC, BC, nine pairs, (qu, qv) from s as in
 * (2); (4) the same point sequence for V = a, b, c against the query triangle (P0, g0, g2), (u, v) = (0, 0), (1, 0), (0, 1), (qu, qv) the
 * clamp of what it returns; (5) the form of (2) with the roles exchanged: normal cross3(g0, g2), heights from P0, the scene's edges
 * (a, b), (a, c), (b, c) as differences of those points, the crossing against (P0, g0, g2); (u, v) = (s, 0), (0, s), (1 - s, s), (qu, qv)
 * as in (4).  A later feature replaces an earlier one only when its d2 is strictly smaller; a feature with a NaN d2 is skipped, a
 * triangle all of whose features are NaN is never a candidate.  The value depends on the record, the instance record and the packet
 * only, never on the tree.
 * Points: a record with P0 == P1 == P2 in all components is answered by feature (1) for P0 alone: its rt_hit is
 * rt_closest_point_device's record for (P0, r_max) byte for byte, and qu = qv = 0.
 * Edges: features (1) to (3) are the union of rt_closest_segment_device's features for the three records (Pi, r_max, Pj) of the edges
 * above, so d2 never exceeds the d2 of any of the three and t <= t_edge holds exactly; when the winning feature is one of (1) to (3) the
 * record equals the best of the three edge records in (t, inst, prim, u, v).  A record with two equal vertices is not promised the
 * bytes of a segment record.
 * Pierced and touching triangles: a scene triangle that cuts or touches the query triangle reports the rounding residue of a crossing
 * feature, a t around 2^-24 of the scene's magnitude, not an exact 0: compare t with a tolerance, or ask rt_overlap_triangles_device.
 * Among several the key decides.
 * d_attr (optional): n rt_hit_attr, 16-B aligned: what rt_closest_point_device gives for (inst, prim, u, v) — P the surface point, N the
 * interpolated shading normal, objectIndex; a miss zeros and -1.  `reserved` is the side of the scene triangle's plane the query's
 * point (P0 + qu g0) + qv g2 lies on (per component two products and two sums in that order), by rt_closest_point_device's rule
 * (FLIP_FACING included), 0 on a miss.
 * Stream ordering without host synchronisation, the TLAS and scene of the call, the query workspace, queries and shading calls of one
 * context one after another, RT_ERR_NOT_READY and n == 0 (nothing is enqueued): as for rt_closest_point_device.
 * RT_ERR_INVALID_ARGUMENT: a NULL pointer (d_attr and d_params aside), a misaligned pointer, a pointer that is not memory of ctx's GPU,
 * n >= 0xFFFFFF00, cull_mask > 0xFF, trace_variant != 0. */
int rt_closest_triangle_device(rt_ctx* ctx, size_t n, const void* d_tris12, uint32_t cull_mask,
                               void* d_hits, void* d_attr, void* d_params, void* hip_stream);
/* The blocking host form, as rt_closest_segment is to rt_closest_segment_device; params_host, when given, takes n x 2 floats. */
int rt_closest_triangle(rt_ctx* ctx, size_t n, const float* tris12_host, uint32_t cull_mask,
                        rt_hit* out_host, float* params_host, int counting, rt_stats* stats);

/* Triangles of the scene as the query, by (inst, prim) reference: the two triangle queries above asked about bodies of the scene
 * itself ("does body 5 touch anything", "the clearance between link 3 and link 7") without a second copy of the mesh, without spending
 * mask bits on self-exclusion, and for one pair of instances without walking the TLAS.
 * References: d_refs4 holds n records of 16 B, 16-B aligned, memory of ctx's GPU; one buffer feeds all three calls. */
typedef struct rt_tri_ref {
  int32_t inst;     /* source instance: index into the context's current instance array */
  int32_t prim;     /* source triangle: gl_PrimitiveID within that instance's mesh */
  int32_t against;  /* RT_REF_AGAINST_OTHERS (-1): candidates from every instance except `inst`;
                       >= 0: candidates from that instance only */
  float   r_max;    /* search radius of rt_closest_scene_triangle_device; ignored by the overlap query */
} rt_tri_ref;
#define RT_REF_AGAINST_OTHERS (-1)
/* The query triangle of a valid record is the world image of the source packet in the arithmetic of the candidate side: v0, v1, v2 from
 * the scene's vertex buffer through the instance's mesh range (after rt_refit_blas_device: the refitted vertices), e1 = v1 - v0 and
 * e2 = v2 - v0 each rounded once, P0 = xform_point(o2w, v0), P1 = P0 + xform_vec(o2w, e1), P2 = P0 + xform_vec(o2w, e2): exactly the
 * (A, B, C) of the canonical predicates for that instance and packet.
 * An invalid record is no error.  It is answered as the plain calls answer a record with a non-finite vertex: the overlap query gives
 * count 0 and an empty row, the distance query the miss record with t = r_max as given.  A record is invalid when inst is outside
 * [0, n_instances), prim is outside [0, triangles of the instance's mesh) (a mesh without triangles has no valid prim), against < -1 or
 * against >= n_instances, the source triangle is a BAD TRIANGLE (rt_upload_geometry), or a coordinate of the world image is not finite
 * (a source instance with a non-finite transform).  Nothing else about the source matters: its mask, its flags and cull_mask play no
 * part in whether it may ask; a non-invertible or masked-out source with a finite image is a valid query.
 * Candidates: those of the plain call for that world triangle (same predicate, same key, same cull_mask rule, same behaviour of void
 * and non-invertible instances), restricted: with against == -1 the candidate's instance index must differ from inst; with
 * against >= 0 it must equal against, and that instance must still be admitted by cull_mask.  against == inst is not special: the
 * instance's own triangles are candidates, prim itself included.  The restriction removes candidates before the key's minimum or the
 * row is formed; it never changes the test of a remaining pair.
 * Role: the query side and the candidate side play different roles in the canonical sequences, so the record (a, i, against b) and the
 * records of b against a are two different questions and may differ at ties.
 *
 * rt_scene_triangles_device writes the world triangles themselves: n records of 48 B in rt_overlap_triangles_device's layout into
 * d_tris12 (16-B aligned, memory of ctx's GPU): words 0-2, 4-6, 8-10 = P0, P1, P2 (nine quiet NaNs, 0x7FC00000, for an invalid
 * record), word 3 = r_max as given (bit pattern kept), word 7 = the bits of inst, word 11 = the bits of against.  The plain triangle
 * calls ignore words 7 and 11, so the output feeds them directly, rt_overlap_boxes_device on its bounds, and drawing.
 * Stream ordering, the TLAS and scene of the call, RT_ERR_NOT_READY and n == 0: as for rt_overlap_triangles_device.
 * RT_ERR_INVALID_ARGUMENT: a NULL, misaligned or non-device pointer, n >= 0xFFFFFF00, trace_variant != 0. */
int rt_scene_triangles_device(rt_ctx* ctx, size_t n, const void* d_refs4, void* d_tris12, void* hip_stream);
/* rt_overlap_triangles_device with d_refs4 in the place of d_tris12: outputs, max_ids 0..16, RT_OVERLAP_ANY, the pruning without
 * d_counts, the alignment rules, the RT_ERR_INVALID_ARGUMENT list, RT_ERR_NOT_READY, stream ordering without host synchronisation,
 * n == 0 and the query workspace (which also holds the n x 48 B of expanded records; an allocation that fails is
 * RT_ERR_OUT_OF_MEMORY and leaves the context as it was) are the plain call's.  Ids and counts name the candidate triangle. */
int rt_overlap_scene_triangles_device(rt_ctx* ctx, size_t n, const void* d_refs4, uint32_t cull_mask, uint32_t flags,
                                      uint32_t max_ids, void* d_ids, void* d_counts, void* hip_stream);
/* The blocking host form, as rt_overlap_triangles is to rt_overlap_triangles_device; the expansion is inside the timed window. */
int rt_overlap_scene_triangles(rt_ctx* ctx, size_t n, const rt_tri_ref* refs_host, uint32_t cull_mask, uint32_t flags,
                               uint32_t max_ids, int32_t* ids_host, uint32_t* counts_host, int counting, rt_stats* stats);
/* rt_closest_triangle_device with d_refs4 in the place of d_tris12, in the same way.  The hit names the candidate triangle; (qu, qv)
 * and the side word of d_attr refer to the source triangle's world image. */
int rt_closest_scene_triangle_device(rt_ctx* ctx, size_t n, const void* d_refs4, uint32_t cull_mask,
                                     void* d_hits, void* d_attr, void* d_params, void* hip_stream);
/* The blocking host form, as rt_closest_triangle is to rt_closest_triangle_device. */
int rt_closest_scene_triangle(rt_ctx* ctx, size_t n, const rt_tri_ref* refs_host, uint32_t cull_mask,
                              rt_hit* out_host, float* params_host, int counting, rt_stats* stats);

/* Overlap lists: every candidate of every record, for the consumers that want all pairs (Embree's rtcCollide, FCL's collide, PhysX's
 * overlap buffers, voxelisers, cutters), where the three calls above give a count and the 16 smallest.  The result is in CSR form:
 *   d_offsets   n + 1 uint64, 8-byte aligned.  offsets[i] is the sum of |C(j)| over j < i and offsets[n] the total T.  The offsets
 *               are always complete: capacity never limits them.  (64 bits: n and every count are below 2^32, their sum is not.)
 *   d_ids       capacity records of 8 bytes (int32 inst, int32 prim), 4-byte aligned.  Row i is the whole of C(i) in ascending
 *               (inst, prim) order at ids[offsets[i] .. offsets[i + 1]).  A row is written if and only if offsets[i + 1] <= capacity:
 *               a row that would cross the capacity, and every row behind it, is not written at all.  No byte at or beyond
 *               min(T, capacity) records is touched, nor any byte of a row that is not written.  The caller compares offsets[n] with
 *               capacity and calls again with more room if it has to.  capacity == 0 wants d_ids == NULL and gives the offsets only.
 * The records, their validity rules (an invalid record has an empty row), the candidates C, the cull mask, the `against` rule of
 * references and the canonical predicates are exactly those of rt_overlap_boxes_device, rt_overlap_triangles_device and
 * rt_overlap_scene_triangles_device.  So the first min(|C(i)|, 16) entries of row i are the row of that call with max_ids = 16, byte for
 * byte, offsets[i + 1] - offsets[i] is its count, and the result is the same bytes whatever the tree.
 * No flag is defined: RT_OVERLAP_ANY and unknown bits are RT_ERR_INVALID_ARGUMENT, and so are a NULL or misaligned pointer (the
 * records 16-byte aligned), memory that is not of ctx's GPU, n >= 0xFFFFFF00, capacity >= 0xFFFFFF00 (rows are indexed with 32 bits
 * once they are known to fit), d_ids == NULL with capacity != 0 or d_ids != NULL with capacity == 0, cull_mask > 0xFF and
 * trace_variant != 0.
 * Stream ordering without host synchronisation, the TLAS and scene of the call, RT_ERR_NOT_READY and "queries of one context one
 * after another" are as for rt_overlap_boxes_device; for n == 0 nothing is enqueued and d_offsets is not written.  A call walks twice:
 * the count-only walk of the capped call, a scan of the counts, then (capacity != 0) a second walk that writes the rows and a sort of
 * the longer rows.  The counts, the scan's storage and the sort's worklist (about 8 n bytes) are part of the query workspace;
 * it grows after the context's earlier queries are done, and an allocation that fails is RT_ERR_OUT_OF_MEMORY and leaves the context as
 * it was. */
int rt_overlap_boxes_device_list(rt_ctx* ctx, size_t n, const void* d_boxes8, uint32_t cull_mask, uint32_t flags,
                                 void* d_offsets, void* d_ids, size_t capacity, void* hip_stream);
int rt_overlap_triangles_device_list(rt_ctx* ctx, size_t n, const void* d_tris12, uint32_t cull_mask, uint32_t flags,
                                     void* d_offsets, void* d_ids, size_t capacity, void* hip_stream);
int rt_overlap_scene_triangles_device_list(rt_ctx* ctx, size_t n, const void* d_refs4, uint32_t cull_mask, uint32_t flags,
                                           void* d_offsets, void* d_ids, size_t capacity, void* hip_stream);
/* The blocking host forms, as rt_overlap_boxes is to rt_overlap_boxes_device: offsets_host (n + 1) and ids_host (capacity pairs; NULL
 * with capacity 0) are host memory, and the entries of ids_host that the call does not write keep their values.  counting != 0 runs the
 * instrumented walks and returns stats->node_visits and stats->tri_tests: those of both walks together (of the one walk with capacity
 * 0); stats may be NULL.  stats->ms_trace_closest is the device time of the whole sequence (for references the expansion too); the size
 * fields as for rt_overlap_boxes. */
int rt_overlap_boxes_list(rt_ctx* ctx, size_t n, const float* boxes8_host, uint32_t cull_mask, uint32_t flags,
                          uint64_t* offsets_host, int32_t* ids_host, size_t capacity, int counting, rt_stats* stats);
int rt_overlap_triangles_list(rt_ctx* ctx, size_t n, const float* tris12_host, uint32_t cull_mask, uint32_t flags,
                              uint64_t* offsets_host, int32_t* ids_host, size_t capacity, int counting, rt_stats* stats);
int rt_overlap_scene_triangles_list(rt_ctx* ctx, size_t n, const rt_tri_ref* refs_host, uint32_t cull_mask, uint32_t flags,
                                    uint64_t* offsets_host, int32_t* ids_host, size_t capacity, int counting, rt_stats* stats);

/* Instance pairs: the two by-reference queries one level up, per pair of bodies (FCL's distance and collide, PhysX's computePenetration,
 * Bullet's closest points, Embree's rtcCollide): "the clearance between link 3 and link 7 and where", "does body 5 touch anything".  A
 * record stands for every triangle of its source instance; the caller builds no reference per triangle, keeps no n x P records and
 * reduces nothing.  Both calls are defined entirely through rt_closest_scene_triangle_device and rt_overlap_scene_triangles_device, so
 * their results are the same bytes whatever the tree.
 * Records: d_irefs4 holds n records of 16 B, 16-B aligned, memory of ctx's GPU; one buffer feeds both calls. */
typedef struct rt_inst_ref {
  int32_t inst;      /* source instance: index into the context's current instance array */
  int32_t against;   /* RT_REF_AGAINST_OTHERS (-1) or a candidate instance, as in rt_tri_ref */
  float   r_max;     /* search radius of the distance query; ignored by the overlap query */
  uint32_t reserved; /* ignored */
} rt_inst_ref;
/* Validity: a record is valid when inst is in [0, n_instances) and against is in [-1, n_instances); the distance query also wants
 * r_max >= 0 and not NaN.  An invalid record is no error, and neither is a source mesh without triangles or a source all of whose
 * triangles are invalid references (BAD TRIANGLES, a non-finite transform): the distance query answers the miss form, the overlap
 * query count 0 and first (-1, -1, -1, 0).  Everything else is the by-reference calls': against == inst is not special, cull_mask
 * admits candidates only (the source's mask plays no part), void and non-invertible records behave as they do there.
 *
 * rt_closest_instances_device.  For a valid record let R_p be the record rt_closest_scene_triangle_device gives the reference
 * (inst, p, against, r_max) under the same cull_mask, p = 0 .. P - 1 (P the triangles of the source's mesh), and d2_p its canonical d2
 * (the key is d2, not the rounded t, as everywhere in the family).  The answer is R_p*, p* the smallest p among those with the smallest
 * d2_p:
 *   d_hits[i]       that hit (4-B aligned): the candidate's inst and prim, its u and v, t = sqrtf(d2);
 *   d_src_prims[i]  p* (int32, 4-B aligned, required);
 *   d_params        (optional, n x 2 floats, 4-B aligned) its (qu, qv), on the world image of source triangle p*;
 *   d_attr          (optional, n rt_hit_attr, 16-B aligned) its attributes, the side word included;
 * all of them byte for byte what rt_closest_scene_triangle_device returns for (inst, p*, against, r_max).  When no source triangle has a
 * candidate: the miss record with t = r_max as given (bit pattern kept), src_prim -1, parameters 0, attributes of a miss.
 *
 * rt_overlap_instances_device.
 *   d_counts64[i]   (uint64, 8-B aligned, required) the sum over p of the count rt_overlap_scene_triangles_device gives (inst, p, against):
 *                   the number of intersecting triangle pairs (64 bits: every count is below 2^32, their sum is not);
 *   d_first4        (optional, n x 4 int32, 4-B aligned) (p, inst, prim, 0): p the smallest source primitive with a non-empty row,
 *                   (inst, prim) the first entry of that row; (-1, -1, -1, 0) when there is none.
 * RT_OVERLAP_ANY in flags makes d_counts64[i] 0 or 1, and the walk of a whole record ends at the first contact any of its source
 * triangles finds; d_first4 must then be NULL, because which pair ends the walk is not deterministic.
 *
 * Stream ordering without host synchronisation, the TLAS and scene of the call, queries and shading calls of one context one after
 * another, RT_ERR_NOT_READY and n == 0 (nothing is enqueued): as for rt_closest_point_device.  A call plans (the work items of every
 * record and a scan of them; their total stays on the device), walks every source triangle as one work item, the items of a record
 * sharing one bound (distance) or one flag (RT_OVERLAP_ANY), and finishes with the by-reference call over one reference per record.
 * The plan, the keys and those references (about 50 n bytes, and n x 48 B of expanded records) are part of the query workspace; it
 * grows after the context's earlier queries are done, and an allocation that fails is RT_ERR_OUT_OF_MEMORY and leaves the context as it
 * was.
 * RT_ERR_INVALID_ARGUMENT: a NULL pointer (d_attr, d_params and d_first4 aside), a misaligned pointer, memory that is not of ctx's GPU,
 * n >= 0xFFFFFF00 or n x (the largest triangle count of any mesh of the scene) >= 0xFFFFFF00 (work items are indexed with 32 bits and
 * the records live on the device, so the check is conservative), unknown flag bits, d_first4 with RT_OVERLAP_ANY, cull_mask > 0xFF,
 * trace_variant != 0. */
int rt_closest_instances_device(rt_ctx* ctx, size_t n, const void* d_irefs4, uint32_t cull_mask,
                                void* d_hits, void* d_src_prims, void* d_attr, void* d_params, void* hip_stream);
int rt_overlap_instances_device(rt_ctx* ctx, size_t n, const void* d_irefs4, uint32_t cull_mask, uint32_t flags,
                                void* d_counts64, void* d_first4, void* hip_stream);
/* The blocking host forms, as rt_closest_scene_triangle and rt_overlap_scene_triangles are to their device calls: out_host,
 * src_prims_host and counts_host are required, params_host and first4_host optional.  counting != 0 runs the instrumented walks and
 * returns stats->node_visits and stats->tri_tests summed over all walks of the call (the finish included); stats->ms_trace_closest is
 * the device time of the whole sequence.  The visits of a shared-bound or shared-flag walk depend on the order in which the lanes of a
 * record publish, that is on timing: the counts are for measurement, not for tests of equality.  The results never depend on it. */
int rt_closest_instances(rt_ctx* ctx, size_t n, const rt_inst_ref* irefs_host, uint32_t cull_mask,
                         rt_hit* out_host, int32_t* src_prims_host, float* params_host, int counting, rt_stats* stats);
int rt_overlap_instances(rt_ctx* ctx, size_t n, const rt_inst_ref* irefs_host, uint32_t cull_mask, uint32_t flags,
                         uint64_t* counts_host, int32_t* first4_host, int counting, rt_stats* stats);

/* Instance broad phase: which bodies can be within a margin of which (the sweep-and-prune or grid in front of FCL's collide, PhysX's
 * broad phase), asked of the TLAS the context already holds and answered in the record format the two calls above read: one buffer
 * feeds the next call.  The caller computes no world box of a mesh the library holds.
 * Records: n rt_inst_ref as they are.  r_max is the margin m: the search radius a later rt_closest_instances_device will use, 0 for
 * contact, +inf allowed.  reserved is ignored.  A source record is valid when inst is in [0, n_instances), against is in
 * [-1, n_instances), r_max >= 0 and not NaN, the source instance is not void (rt_set_instances) and its mesh has an active triangle.
 * An invalid record has an empty row and is no error.  The source's own mask plays no part; a non-invertible record with a finite
 * transform is valid, as in the world-space queries.
 * The canonical box of instance i depends on its record and its mesh only, never on a tree or on another instance.  [lo, hi] are the
 * exact binary32 bounds of the vertices of the mesh's active triangles and M is the record's transform.  The eight corners of [lo, hi]
 * are mapped in binary64, M_r0 p0 + M_r1 p1 + M_r2 p2 + M_r3 in that order, each coordinate rounded once to binary32; blo and bhi are
 * their bounds.  With bm_k = max(|lo_k|, |hi_k|) and mw = max_r (|M_r0| bm_0 + |M_r1| bm_1 + |M_r2| bm_2 + |M_r3|) in binary32, unfused,
 * left to right, Box(i) = [blo - e, bhi + e], e = 2^-13 mw, every bound rounded once.  An instance one of whose three row sums is not
 * finite has no box: it is in no row and its own rows are empty.
 * Candidates of record (i, against, m): instance j when it has a box, (its mask & cull_mask) != 0 (a void record and an instance of
 * an empty mesh have mask 0), j != i when against == -1, j == against when against >= 0 (against == inst is not special), j > i with
 * RT_INSTANCE_PAIRS_ABOVE in flags, and on every axis k both !(Box(i).lo_k - m > Box(j).hi_k) and !(Box(i).hi_k + m < Box(j).lo_k),
 * the two inflated values rounded once in binary32.  The test is closed: touching boxes count.
 * Output, in CSR form with the rules of rt_overlap_*_device_list: d_offsets is n + 1 uint64, 8-byte aligned, always complete; d_pairs4 is
 * capacity records of 16 B, 16-byte aligned.  Row i holds (inst of record i, j, r_max of record i with its bit pattern kept, 0) for
 * every candidate j in ascending j, and is written if and only if offsets[i + 1] <= capacity.  No byte of a row that is not written, or
 * at or beyond min(T, capacity) records, is touched.  capacity == 0 wants d_pairs4 == NULL and gives the offsets only.  The rows are
 * valid input of rt_closest_instances_device and rt_overlap_instances_device as they are.
 * GUARANTEE: under the same cull_mask, every j for which rt_overlap_instances_device counts a pair for (i, j), or for which
 * rt_closest_instances_device returns a hit for (i, j, m), is in the row of (i, -1, m) (DESIGN.md §5 "Instance broad phase": the slack e
 * covers the rounding of every world vertex the narrow phase makes).  With RT_INSTANCE_PAIRS_ABOVE and every instance asking, every
 * unordered pair is listed once.
 * Stream ordering without host synchronisation, the TLAS and scene of the call, "queries of one context one after another", the
 * workspace (the list calls' and 32 bytes per instance) and RT_ERR_OUT_OF_MEMORY, RT_ERR_NOT_READY and n == 0 (nothing is enqueued,
 * d_offsets is not written) are as for the list calls.  RT_ERR_INVALID_ARGUMENT: a NULL or misaligned pointer, memory that is not of
 * ctx's GPU, n or capacity >= 0xFFFFFF00, d_pairs4 == NULL with capacity != 0 or the reverse, unknown flag bits, cull_mask > 0xFF,
 * trace_variant != 0. */
#define RT_INSTANCE_PAIRS_ABOVE 0x1u   /* list only candidates j > inst: every unordered pair once when every instance asks */
int rt_instance_pairs_device(rt_ctx* ctx, size_t n, const void* d_irefs4, uint32_t cull_mask, uint32_t flags,
                             void* d_offsets, void* d_pairs4, size_t capacity, void* hip_stream);
/* The blocking host form, as rt_overlap_boxes_list is to its device call: the entries of pairs_host that the call does not write keep
 * their values.  counting != 0 returns stats->node_visits (TLAS node visits) and stats->tri_tests (exact box-pair tests) of all walks;
 * stats->ms_trace_closest is the device time of the whole sequence. */
int rt_instance_pairs(rt_ctx* ctx, size_t n, const rt_inst_ref* irefs_host, uint32_t cull_mask, uint32_t flags,
                      uint64_t* offsets_host, rt_inst_ref* pairs_host, size_t capacity, int counting, rt_stats* stats);

/* Inside / outside: for every point, is it enclosed by the scene's surfaces (Open3D's compute_occupancy and compute_signed_distance),
 * for signed distance fields, penetration tests, occupancy and voxel filling.  The answer is a vote over the crossing parities of a few
 * rays from the point along a fixed table of generic directions; one ray is not enough, because the canonical triangle test is not
 * watertight (a ray through a shared edge or vertex may be counted by both triangles or by neither), and three are (DESIGN.md §5
 * "Inside / outside").
 * Points: d_points4 holds n records of 16 B (x, y, z, w), 16-B aligned, memory of ctx's GPU: rt_closest_point_device's record.
 * rt_point_inside* ignores w, so one buffer feeds both queries.
 * Directions: n_dirs is 1, 3 or 5, the first n_dirs rows of RT_INSIDE_DIRS below, as these decimal literals round to binary32; they
 * are used as given, not normalised.
 * Crossing count: count_k(p) is the value rt_intersect_device_hits writes to d_counts for the ray (p, tmin 0, D_k, tmax +inf) with
 * max_hits 0, ray_flags 0 and the call's cull_mask: its candidates, its instance mask rule, its object-space transform of the ray and
 * the canonical triangle test.  Instance flags, opacity and facing play no part.  It depends on the point, the instance records and the
 * packets only, never on the tree.
 * Vote: the directions are taken in order k = 0, 1, ...; the walk stops as soon as odd or even holds more than n_dirs / 2 votes.
 * d_inside: n uint32, 4-B aligned.  Word i: bit 0 is 1 when odd won (the point is inside); bits 8-15 the number of odd votes among the
 * directions taken; bits 16-23 the number of directions taken.  The word is a function of the counts alone.
 * d_counts (optional): n x n_dirs uint32, point-major, 4-B aligned: count_k of every direction.  Then every direction is taken: bits
 * 16-23 read n_dirs, bits 8-15 count the odd votes among all of them, and bit 0 is the same either way.
 * A point with a non-finite coordinate gets word 0 and counts 0.
 * Stream ordering without host synchronisation, the TLAS and scene of the call, the query workspace, queries and shading calls of one
 * context one after another, RT_ERR_NOT_READY and n == 0 (nothing is enqueued): as for rt_closest_point_device.
 * RT_ERR_INVALID_ARGUMENT: a NULL (d_counts aside) or misaligned pointer, a pointer that is not memory of ctx's GPU, n >= 0xFFFFFF00,
 * n x n_dirs >= 0xFFFFFF00 when d_counts is given, cull_mask > 0xFF, n_dirs not 1, 3 or 5, trace_variant != 0. */
#define RT_INSIDE_MAX_DIRS 5
#define RT_INSIDE_DIRS { {0.36f, 0.48f, 0.8f}, {-0.8f, 0.36f, -0.48f}, {0.48f, -0.8f, -0.36f}, {-0.6f, -0.64f, 0.48f}, {0.64f, -0.48f, 0.6f} }
int rt_point_inside_device(rt_ctx* ctx, size_t n, const void* d_points4, uint32_t cull_mask, uint32_t n_dirs,
                           void* d_inside, void* d_counts, void* hip_stream);
/* The blocking host form, as rt_closest_point is to rt_closest_point_device: the points are copied to the device, voted on the
 * context's stream (same workspace and ordering) and the words (and counts, when counts_host is not NULL) copied back.  counting != 0
 * runs the instrumented walk and fills stats->node_visits and stats->tri_tests; stats may be NULL.  As rt_sweep_spheres does, the call
 * also reports the walk's device time in stats->ms_trace_closest and the node and packet sizes in stats->bvh_node_bytes /
 * bvh_tri_bytes; every other field is 0. */
int rt_point_inside(rt_ctx* ctx, size_t n, const float* points4_host, uint32_t cull_mask, uint32_t n_dirs,
                    uint32_t* inside_host, uint32_t* counts_host, int counting, rt_stats* stats);
/* Signed distance: rt_closest_point_device and the vote above in one call, under one ordering.  d_hits and d_attr receive
 * rt_closest_point_device's records for (x, y, z, r_max) byte for byte, except the sign bit of t, which is set when bit 0 of the point's
 * word is set: a point inside has t <= -0.0, the miss record of a point inside is -r_max, and t = 0 becomes -0.0.  A record that is not
 * a valid closest-point query (a non-finite coordinate, a negative or NaN r_max) keeps its miss form unchanged.
 * d_inside (optional): n uint32, the early-stop words of rt_point_inside_device.
 * Everything else, RT_ERR_INVALID_ARGUMENT included: as for rt_closest_point_device and rt_point_inside_device. */
int rt_signed_distance_device(rt_ctx* ctx, size_t n, const void* d_points4, uint32_t cull_mask, uint32_t n_dirs,
                              void* d_hits, void* d_attr, void* d_inside, void* hip_stream);

/* Custom ray generation: the frame's shading of the caller's primary rays.  The caller's rays replace the pinhole camera of
 * src/shader.rgen:62-82; everything after it — the bounce loop of src/shader.rgen:84-177 with closest hit, miss, reflection, refraction and
 * shadow rays — is the frame's, and the colours are those a frame would compute for the same rays.
 * Rays: d_rays8 holds n = n_points * n_samples records of 32 B in rt_intersect's layout (o.xyz, w3, d.xyz, tmax), 16-B aligned, memory of
 * ctx's GPU, sample-major: record i * n_points + p is sample i of point p (a frame's sample id i * pixels + p).  The sample index i gives
 * the pow(0.9, i) weight of src/shader.rgen:127; n_samples = 1 is plain per-ray shading.  The first segment is traced over
 * [0.001, tmax] (tmax = 10000 is src/shader.rgen:87); word 3 is ignored.  Every later segment and every shadow ray uses the reference's
 * constants.  Directions are used as given, like rayDirection after the normalize of src/shader.rgen:81: the caller normalises them.
 * A record with a non-finite component in o or d, or with d = 0, is not traced: its sample is (0, 0, 0, 0) — alpha 0 marks it — and it
 * still counts in its point's average.  tmax <= 0.001 (or NaN) is an empty interval: a miss, the sample is the sky colour.
 * Scene and uniforms are the context's, as for a frame: instances, BLASes, materials, instance types, skybox, light position and
 * intensity, maxBounceCount, the object types.  The camera fields and samplesPerPixel are ignored.
 * Outputs (at least one; float32 RGBA, 16-B aligned, memory of ctx's GPU): d_sample_rgba, optional, n float4 — each sample's tmpColor
 * with alpha 1, the color += vec4(tmpColor, 1) term of src/shader.rgen:178; d_point_rgba, optional, n_points float4 — the average of a
 * point's samples with the frame's ordered sum and division (src/shader.rgen:178-183).  The pinhole rays of a frame therefore give the
 * frame bit for bit.  output_rgba8 / output_bgra8 do not apply.
 * Ordering as rt_intersect_device: rays are read and outputs written in stream order on hip_stream (NULL = the context's stream); no host
 * copy, no host synchronisation, no wait for a frame in flight on the context (the call has queues of its own, allocated at the first
 * call and grown after the previous call is done).  The call sees the TLAS of the last rt_set_instances* before it and the scene as it
 * was at the call; shading calls and device ray queries of a context run one after another.  n_points == 0 enqueues nothing.  The call
 * is not counted in rt_get_stats.
 * RT_ERR_INVALID_ARGUMENT: NULL ctx, NULL rays with n > 0, both outputs NULL, a misaligned pointer or one that is not device memory of
 * ctx's GPU, n_samples == 0, n > 2^25, a maxBounceCount a frame refuses, trace_variant != 0; RT_ERR_NOT_READY: as for a frame (no uniforms, no
 * geometry, no TLAS, a TLAS stale after rt_refit_blas_device, a frame batch held by the context). */
int rt_shade_rays_device(rt_ctx* ctx, size_t n_points, uint32_t n_samples, const void* d_rays8, void* d_sample_rgba, void* d_point_rgba, void* hip_stream);

/* Same frame as rt_trace but through the instrumented traversal kernels (visit counters). */
int rt_trace_counting(rt_ctx* ctx, int width, int height, float* out_rgba32f_host, rt_stats* stats);

/* Host-only self check of the acceleration-structure builders (needs no GPU): builds the BVH2 / BVH4 / quantized nodes of
 * an indexed mesh as rt_build_blas(blas_builder 0) does and verifies their invariants (every triangle in exactly one leaf,
 * children inside parents, quantized boxes containing float boxes, depth and stack bounds).  out[8] = nodes, leaves,
 * depth, max leaf size, BVH4 nodes, BVH4 stack need, violations, triangles reached.  0 = all invariants hold. */
int rt_debug_check_builders(const float* verts6, size_t n_floats, const uint32_t* idx, size_t n_idx, uint64_t* out8);
/* Host-only sibling of rt_debug_snapshot (needs no GPU): the quantized BVH2 and the triangle packets that rt_build_blas(blas_builder 0)
 * produces for an indexed mesh, in the device record layouts (32-byte nodes with links local to the mesh, 48-byte packets).  out8 = nodes,
 * packets, q_lo[3], q_scale[3] (binary32 bit patterns).  n triangles give at most max(1, n - 1) nodes and n packets;
 * RT_ERR_INVALID_ARGUMENT on a NULL pointer, an index outside verts6 or a buffer that is too small. */
int rt_debug_host_blas(const float* verts6, size_t n_floats, const uint32_t* idx, size_t n_idx, void* nodes, size_t nodes_capacity_bytes,
                       void* packets, size_t packets_capacity_bytes, uint64_t* out8);
/* TEST HOOK, not a product path: copies to the host, as raw bytes in the device record layouts, what the kernels of ctx read.  Waits for
 * the pending frames, queries and uploads of the scene (as rt_build_blas does), launches no kernel.  what = 0: 20 x uint64 — linked BLAS
 * nodes, tlas_base (global node index of ctx's TLAS region of its current parity), nodes of one TLAS, tlas_stride (0 without a batch),
 * batch_k, triangle packets, instance records (all frames of a batch), instances per frame, meshes, vertex floats, indices, frontier
 * boxes, tlas_q_lo[3], tlas_q_scale[3] (binary32 bit patterns), TLAS nodes item 2 copies (batch_k * tlas_stride for a batch), 0;
 * 1: the linked BLAS nodes; 2: the TLAS region; 3: the triangle packets; 4: the instance records of the current parity; 5: the device
 * mesh table; 6: the device vertex buffer; 7: the device index buffer; 8: the frontier boxes (6 floats each).  *bytes (may be NULL)
 * receives the item's size.  RT_ERR_NOT_READY without a valid TLAS; RT_ERR_INVALID_ARGUMENT: NULL ctx or out, unknown item, capacity_bytes too small. */
int rt_debug_snapshot(rt_ctx* ctx, int what, void* out, size_t capacity_bytes, size_t* bytes);
/* Host-only view of the launch/allocation sizing rules (needs no GPU): out2[0] = workgroups of the k_tail grid on a device
 * of n_cu compute units holding resident_per_cu of them each (0 = k_tail is not used), out2[1] = int32 elements of the
 * spill-stack allocation for that grid, a traversal grid of trace_blocks workgroups and ovf_stride entries per thread. */
int rt_debug_sizing(int n_cu, int resident_per_cu, int trace_blocks, uint32_t ovf_stride, uint64_t* out2);

/* Message of the last failing call on this context (or of rt_create when ctx==NULL). */
const char* rt_last_error(const rt_ctx* ctx);
/* "gfx950 <device name> CUs=<n>" of the bound device. */
const char* rt_device_info(const rt_ctx* ctx);
/* ABI version: bumped on any signature/layout change. */
int rt_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RT_API_H */
