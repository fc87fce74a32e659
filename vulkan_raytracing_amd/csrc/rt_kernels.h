// rt_kernels.h — launch interface between the host library (rt_api.cpp) and kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_device.h"

namespace rt {

struct SceneDev {
  const BvhNodeQ* blas_nodes;  // variant 0: quantized BVH2 nodes of all meshes, then the quantized TLAS nodes
  int tlas_root;               // index of the TLAS root in blas_nodes
  int tlas_nodes;              // nodes of this slot's TLAS (they follow the root)
  int tlas_stride;             // frame batches: frame k's TLAS root is tlas_root + k * tlas_stride (0: no batch)
  uint32_t batch_samples;      // frame batches: sample ids per frame (spp * rows * W): frame of a ray = sample id / batch_samples (0: no batch)
  const float4* tris;          // 3 float4 per TriPacket
  float tlas_q_lo[3], tlas_q_scale[3];
  const WideNodeQ* wide_nodes; // variant 2: 4-ary records, same numbering as blas_nodes
  const Bvh4Node* nodes4;      // quad traversal (variant 1): BLAS BVH4 nodes, then the TLAS BVH4 nodes
  int tlas_root4;              // index of the TLAS root in nodes4
  const InstanceDev* inst;
  const float* verts;          // binding 3 (src/main.cpp:1305-1335)
  const uint32_t* idx;         // binding 2
  const uchar4* sky;           // binding 5: 6 layers RGBA8
  int n_inst;
  int sky_w, sky_h;
  uint32_t ovf_stride;         // spill entries per lane behind the LDS stack, sized from the depth of the trees
  const MaterialDev* materials;   // row n4: MTL material table (NULL / n_materials == 0: the reference's hard-coded constants)
  const uint32_t* prim_material;  // material of every triangle of the index buffer (global primitive number = first_index / 3 + gl_PrimitiveID)
  int n_materials;
  const float* cover_boxes;    // object-space frontier boxes of every mesh (lo[3], hi[3]), InstanceDev::cover_first/count index them
};

struct FrameDev {
  float4* ray_o[2];            // ping-pong ray queues: (o.xyz, tmax) — queue 0 with pixel runs: ONE origin per run (camera, tile), in the slot of the run's first entry
  float4* ray_d[2];            //                        (d.xyz, sample id bits)
  float4* hit_a;               // closest-hit records: (t, u, v, prim bits)
  int32_t* hit_inst;           //                       instance index, -1 = miss
  float4* sh_o;                // shadow queue: (o.xyz, tmax = lightDistance)
  float4* sh_d;                //               (L.xyz, sample id bits)
  float4* sh_c;                //               (tmpColor if the light is visible: rgb, material tag bits)
  float4* sample_color;        // per-sample tmpColor (rgb, 1), index = i*(rows*W) + ly*W + x
  uint32_t* counters;          // rt::CNT_* layout; zero when the frame starts
  uint32_t* counters_next;     // the context's other counter block: k_resolve (the frame's last kernel) zeroes it for the next frame
  int32_t* ovf_stack;          // SceneDev::ovf_stride ints per persistent thread
  unsigned long long* stats_out;   // host-mapped StatSlot block, written by k_resolve (NULL: not wanted)
  uint32_t* fault_total;           // the context's never-reset count of frames whose k_tail gave up (device word)
  uint32_t* hint;              // host-mapped array [CNT_MAX_BOUNCES]: size of every bounce queue, written by k_resolve and
                               // read by the host, unsynchronised, as the launch-strategy hint for the next frame
  float4* out;                 // compact shard image (rows x W RGBA32F; rows x W RGBA8 when out_rgba8 is set)
  int out_rgba8;               // 0: RGBA32F, 1: R8G8B8A8, 2: B8G8R8A8
  uint32_t shard_cap;          // entries per queue shard (queues hold N_SHARDS * shard_cap rays)
  int width, height;           // full frame
  int rows;                    // rows rendered by this shard (compact)
  int band_rows, shard, n_shards;
  // Primary-ray coverage mask of this frame (NULL: off).  Word 0 != 0: every tile may be covered; bit t of the words from 1 on:
  // 8x8-pixel tile t = ty * cover_tiles_x + tx of the FULL frame may be touched by a mesh (k_cover); k_raygen shades the samples
  // of an unmarked tile as misses without testing anything.  cover_next/cover_words: the slot's other mask, zeroed by k_resolve.
  const uint32_t* cover;
  uint32_t* cover_next;
  uint32_t cover_words;
  int cover_tiles_x;
  // Entry lists of this frame's primary rays (NULL: off): record of local tile ty * tiles_x + tx, written by k_entry, read by
  // k_raygen (empty tiles) and by the closest-hit launch of bounce 0 (where the tile's rays start their walk).
  EntryRec* entry;
  // Entry lists of the shadow rays (NULL: off): record ((face * light_tiles) + ty) * light_tiles + tx of the cube around the
  // light; k_shade gives every shadow ray its record index (sh_e), the shadow traversal starts there.
  const EntryRec* light_entry;
  uint32_t* sh_e;              // shadow queue: record index | ENTRY_REVERSE, or ENTRY_FROM_ROOT
  int light_tiles;
  int far_possible;            // LaunchCfg::far of this frame (k_raygen's TLAS test)
  int settle_dead_shadow_rays; // k_shade does not queue a shadow ray whose outcome cannot change its sample (rt_set_param "dead_shadow_rays")
  // (ux, uy) of every sample of this frame size and shard layout (k_jitter_table; NULL: k_raygen evaluates the hash itself)
  const float2* jitter;
  // frame batch (rt_device.h BATCH_MAX): `rows` stays the rows of ONE frame's shard; the buffers hold batch_k of them back to back
  int batch_k;                 // 1: a single frame
  uint32_t out_frame_stride;   // pixels between the shard images of consecutive frames of a batch in `out` (>= rows * width)
  uint32_t cover_view_words;   // words of ONE view's coverage mask (frame k's camera mask starts k * cover_view_words into `cover`)
  // Tile blobs (rt_device.h; NULL: off — always in the product library, which has no tile-blob kernels; the fields stay so that
  // rt_api.o, linked into both libraries, sees one layout).  tile_blob[local tile] = arena slot of the tile's blob or BLOB_NONE (k_blob): k_raygen leaves
  // the tiles that have one to k_tile, which generates their rays itself, walks them in LDS, puts them (ray direction + hit record) at the
  // TOP of their shard's region of bounce queue 0 (Q_TILE_RAYS; k_shade reads both ends) and appends the few that may still hit
  // another instance to queue 0 proper for the global walk.
  uint32_t* tile_blob;
  char* blob_arena;
  uint32_t blob_slots;         // arena capacity (slots of BLOB_SLOT_BYTES): N_SHARDS sub-arenas of blob_slots / N_SHARDS
  uint4* blob_list;            // BLOB_CLASSES x N_SHARDS parts of blob_slots / N_SHARDS entries
  // Pixel runs (kernels_beam.inc; 0: off): bounce queue 0 is NOT compacted — every covered tile with a traced sample owns a run of 64
  // slots per sample row of its k_raygen workgroup (slot = run + 64 * row + pixel of the tile), so that k_beam finds the samples of a
  // pixel together; a slot without a ray has a zero direction and gets HIT_DEAD as its hit record.
  int pixel_runs;
  // ... and the shadow ray of a primary hit takes the slot of its primary ray in sh_o / sh_d / sh_c / sh_e (zero direction: none), for
  // k_beam_shadow; the compact shadow queue of the later bounces then starts sh_base entries up in the same arrays (0: no shadow runs;
  // always in the product library, which has no k_beam_shadow)
  uint32_t shadow_runs;        // 0 / 1
  uint32_t sh_base;
};

// camera of k_cover: the inverse of the basis (right, up, forward) maps a world offset v = P - position to (a.x, a.y, a.z) with
// the primary ray through P having ux = 2.5 a.x / a.z, uy = 2.5 a.y / a.z (src/shader.rgen:74-79)
struct CoverArgs {
  float cam[3];
  float inv[9];
  float kf;                    // 2.5 for the camera (src/shader.rgen:79), 1 for a face of the light cube
  float apex_radius;           // rays pass within this distance of cam (see EntryArgs)
  int width, height, tiles_x, tiles_y;
  int n_inst;
  uint32_t mask_offset;        // words from the start of the frame's mask block to this view's mask (word 0: everything marked)
  int inst_base;               // first instance record of this view (frame batches: the view is a frame, its instances follow the previous frame's)
};
struct CoverViews { CoverArgs v[MAX_VIEWS]; int n; };

// beam of a tile (k_entry): apex cam, directions ux * R + uy * U + kf * F with (a, b, c) = inv * (P - cam) the coordinates of a
// point in the basis (R, U, F); the camera: R, U, F = right, up, forward, kf = 2.5 (src/shader.rgen:79)
struct EntryArgs {
  float cam[3];
  float inv[9];
  float basis[9];              // R, U, F (three vectors): the centre ray of a tile orders its entries
  float kf;
  float apex_radius;           // the rays pass within this distance of cam (0: through it).  Shadow rays start 0.01 N off the surface
                               // point whose direction to the light they take (src/shader.rgen:107-110), so they end 0.01 N off the light
  int width, height;           // full frame
  int tiles_x, tile_rows;      // local tile grid of this shard (= the grid of k_raygen)
  int band_rows, shard, n_shards;
  EntryRec* records;
  const uint32_t* cover;       // coverage mask of this view (tiles it leaves unmarked get an empty record)
  int cover_tiles_x;
  int tlas_root_offset;        // frame batches: this view's (frame's) TLAS root is sc.tlas_root + tlas_root_offset
};
struct EntryViews { EntryArgs v[MAX_VIEWS]; int n; };

// per-frame camera and light of a batch (kernel argument of k_raygen / k_shade / k_tail; frame 0 = the uniform block proper)
struct BatchTab {
  float position[BATCH_MAX][4], right[BATCH_MAX][4], up[BATCH_MAX][4], forward[BATCH_MAX][4];
  float light[BATCH_MAX][4];
};

struct LaunchCfg {
  int trace_blocks;            // persistent grid of the traversal kernels (256 threads each)
  int shade_blocks;
  int rays_per_lane;           // device-side grid sizing of the traversal kernels (see k_trace)
  int min_blocks;
  int variant;                 // 0: BVH2, one lane per ray; 1: BVH4, four lanes per ray; 2: 4-ary records, one lane per ray
  int far;                     // 1: a ray of this frame may be FAR from a tree it walks (kernels.hip quant_far): launch the kernels that carry the far-ray logic
  int packet;                  // variant 0 only.  1: the primary rays (bounce 0) and the shadow rays are walked by k_packet, one wavefront per
                               // 64-ray chunk; 2: the record-level entry (rt_intersect) too (tests: incoherent rays through the packet kernel)
  int packet_blocks;           // persistent grid of k_packet (no LDS, few registers: eight workgroups per CU fit)
};

size_t raygen_block_count(int width, int rows, uint32_t spp, int batch_k);   // workgroups of k_raygen (each appends <= 256 rays to one shard)
void launch_raygen(const SceneDev& sc, const FrameDev& f, const UniformsDev& u, const BatchTab& bt, hipStream_t s);
// the (ux, uy) table k_raygen reads through FrameDev::jitter: jitter_table_elems float2 for (f.width, f.rows, spp) and f's shard layout
size_t jitter_table_elems(int width, int rows, uint32_t spp);
void launch_jitter_table(const FrameDev& f, uint32_t spp, float2* table, hipStream_t s);
// bounce 0 of a frame with entry lists (f.entry) starts every ray at its tile's record
void launch_trace_closest(const SceneDev& sc, const FrameDev& f, int bounce, bool counting, const LaunchCfg& cfg, hipStream_t s);
// bounce 0 of a single frame with pixel runs (f.pixel_runs) and neither counting, tile blobs nor shadow runs: the walk of the primary rays
// and the shading of their hits in one launch (k_beam_shade) — launch_trace_closest + launch_shade of bounce 0, without the hit records
void launch_beam_shade(const SceneDev& sc, const FrameDev& f, const UniformsDev& u, const LaunchCfg& cfg, hipStream_t s);
// one lane per tile of the shard: the record of every tile the coverage mask marks
void launch_entry(const SceneDev& sc, const EntryViews& a, hipStream_t s);
// tile blobs and shadow beams (alt library only; empty in the product library, whose frames never have tile_blob / shadow_runs):
// one wavefront per tile of the camera view `e` (the view the records were made for): the tile's blob
void launch_blob(const SceneDev& sc, const EntryArgs& e, const FrameDev& f, bool counting, hipStream_t s);
// the tiles with a blob: their primary rays generated and walked in LDS, one launch per size class
void launch_tile(const SceneDev& sc, const FrameDev& f, const UniformsDev& u, bool counting, hipStream_t s);
// bounces first_bounce..maxBounceCount (traversal + shading) in one launch of TAIL_BLOCKS workgroups
void launch_tail(const SceneDev& sc, const FrameDev& f, const UniformsDev& u, const BatchTab& bt, int first_bounce, bool counting, const LaunchCfg& cfg, int tail_blocks, hipStream_t s);
void launch_shade(const SceneDev& sc, const FrameDev& f, const UniformsDev& u, const BatchTab& bt, int bounce, const LaunchCfg& cfg, hipStream_t s);
// the shadow rays of the primary hits, one walk per pixel (alt library only, like launch_blob / launch_tile)
void launch_beam_shadow(const SceneDev& sc, const FrameDev& f, const UniformsDev& u, bool counting, const LaunchCfg& cfg, hipStream_t s);
void launch_trace_shadow(const SceneDev& sc, const FrameDev& f, bool counting, const LaunchCfg& cfg, hipStream_t s);
void launch_resolve(const FrameDev& f, const UniformsDev& u, hipStream_t s);
// marks the tiles of `mask` (FrameDev::cover layout) that the frontier boxes of the instances project onto
void launch_cover(const SceneDev& sc, const CoverViews& a, uint32_t max_boxes_per_instance, uint32_t* mask_block, hipStream_t s);
// record-level traceRayEXT (rt_intersect, rt_intersect_device) on the caller's rays, 8 floats each (o.xyz, tmin, d.xyz, tmax), in stream
// order; writes HitRec[n].  counters is a counter block of the query's own (k_query_init writes the ray count and fresh chunk cursors
// into it; counting adds node visits and triangle tests to it, so the caller zeroes it first) and ovf_stack a spill area sized like the
// context's.  cfg.variant and cfg.packet >= 2 choose the alt library's kernels; the product library walks the one-lane BVH2.
void launch_query(const SceneDev& sc, const float4* rays, HitRec* out, uint32_t n, int32_t* ovf_stack, uint32_t* counters, bool any_hit,
                  bool counting, const LaunchCfg& cfg, hipStream_t s);
// rt_hit_attr (two float4) of every closest hit of `hits`
void launch_hit_attr(const SceneDev& sc, const HitRec* hits, float4* attr, uint32_t n, hipStream_t s);
// rt_intersect_device_flags: launch_query with per-ray flags and cull masks; words (n uint32, or null: every word 0xFF000000) and
// query_word (the call's flags | cull mask << 24) combine as the header documents
void launch_query_flags(const SceneDev& sc, const float4* rays, const uint32_t* words, uint32_t query_word, HitRec* out, uint32_t n,
                        int32_t* ovf_stack, uint32_t* counters, const LaunchCfg& cfg, hipStream_t s);
// the hit kind (0xFE front, 0xFF back, 0 miss) of every hit of `hits` into word 7 of its rt_hit_attr (after launch_hit_attr)
void launch_hit_kind(const SceneDev& sc, const float4* rays, const HitRec* hits, float4* attr, uint32_t n, hipStream_t s);
// rt_intersect_device_hits: the k (0..16) nearest accepted candidates of every ray, sorted by (t, inst, prim), into hits (n * k records,
// ray-major; the rest of a row in the miss form), their number into counts (optional: without it the walk prunes by the k-th entry), and
// with attr (k >= 1) the rt_hit_attr of every record with its hit kind.  Rays, words and query_word as for launch_query_flags; the
// walk's chunk cursor is a word of `counters`, its stack spills into ovf_stack (sized for cfg.trace_blocks workgroups).
void launch_query_hits(const SceneDev& sc, const float4* rays, const uint32_t* words, uint32_t query_word, uint32_t n, uint32_t k, HitRec* hits,
                       float4* attr, uint32_t* counts, int32_t* ovf_stack, uint32_t* counters, const LaunchCfg& cfg, hipStream_t s);
// The nearest-pair walks (walk_nearest.inc), one launch for the family: for every record the nearest pair of a point of the record and a
// point of the surface of the instances the cull mask admits, within the record's radius r_max (word 3), into hits[n].
//   Point     rt_closest_point_device: 16 bytes (p.xyz, r_max); no params (kernels_closest.inc)
//   Segment   rt_closest_segment_device: 32 bytes (P0.xyz, r_max, P1.xyz, ignored); params[n]: the segment's parameter s (kernels_segment.inc)
//   Triangle  rt_closest_triangle_device: 48 bytes (P0.xyz, r_max, P1.xyz, ignored, P2.xyz, ignored); params[2 n]: the barycentrics
//             (qu, qv) of the query's point (kernels_triangle.inc)
//   Refs      rt_closest_scene_triangle_device: Triangle over launch_refs_expand's records, honouring words 7 (the source instance) and
//             11 (against: -1 every other instance, >= 0 that one only) (kernels_refs.inc)
// params is optional (null: not written).  inst_scale: 1 + sc.n_inst floats that launch_closest_scale fills first, in stream order ([0]
// the largest row-term magnitude of any instance's o2w, [1 + i] a lower bound on the smallest singular value of instance i's).  Chunk
// cursor, counters (counting: node visits and triangle tests, the caller zeroes the block first) and spill area as for launch_query_hits.
enum class NearestShape { Point, Segment, Triangle, Refs };
void launch_nearest(NearestShape shape, const SceneDev& sc, const float4* records, uint32_t cull_mask, const float* inst_scale, HitRec* hits, float* params, uint32_t n,
                    int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s);
void launch_closest_scale(const SceneDev& sc, float* inst_scale, hipStream_t s);
// the side of the reported triangle's plane every point lies on (0xFE front, 0xFF back, 0 miss) into word 7 of its rt_hit_attr (after launch_hit_attr)
void launch_closest_side(const SceneDev& sc, const float4* points, const HitRec* hits, float4* attr, uint32_t n, hipStream_t s);
// rt_closest_point_device_hits: the k (0..16) nearest candidates of every point (launch_nearest's Point records and candidates), sorted by
// (d2, inst, prim), into hits (n * k records, point-major, t = sqrtf(d2); the rest of a row in the miss form), their number into counts
// (optional: without it the walk prunes by the k-th entry's d2), and with attr (k >= 1) the rt_hit_attr of every record with its side
// word (kernels_closest_hits.inc).  inst_scale, chunk cursor, counters (counting) and spill area as for launch_nearest.
void launch_closest_hits(const SceneDev& sc, const float4* points, uint32_t cull_mask, const float* inst_scale, uint32_t n, uint32_t k, HitRec* hits, float4* attr,
                         uint32_t* counts, int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s);
// The overlap walks (walk_overlap.inc), one launch for the family: for every record the triangles its canonical predicate does not
// separate from it, among the instances the cull mask admits: the k smallest (inst, prim) of each record into ids[n * k] (8 bytes each;
// k == 0: none), their number into counts[n] (or null: the walk prunes); any: counts of 0 or 1, a record ends at its first candidate.
//   Boxes      rt_overlap_boxes_device: 32 bytes (lo.xyz, w3, hi.xyz, w7), the triangles that touch the box (kernels_overlap.inc)
//   Triangles  rt_overlap_triangles_device: 48 bytes (P0.xyz, w3, P1.xyz, w7, P2.xyz, w11), the triangles that cut or touch the query
//              triangle (kernels_triangles.inc)
//   Refs       rt_overlap_scene_triangles_device: Triangles over launch_refs_expand's records, honouring words 7 (the source instance)
//              and 11 (against: -1 every other instance, >= 0 that one only) (kernels_refs.inc)
// inst_scale as for launch_nearest (launch_closest_scale fills it first); chunk cursor, counters (counting) and spill area as for
// launch_query_hits.
enum class OverlapShape { Boxes, Triangles, Refs };
void launch_overlap(OverlapShape shape, const SceneDev& sc, const float4* records, uint32_t cull_mask, const float* inst_scale, bool any, uint32_t k, void* ids,
                    uint32_t* counts, uint32_t n, int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s);
// rt_sweep_spheres_device: the first contact of every moving sphere (32 bytes: o.xyz, r, d.xyz, tmax) with the instances the cull mask
// admits, into hits[n] (kernels_sweep.inc).  inst_scale as for launch_nearest (launch_closest_scale fills it first); chunk cursor,
// counters (counting) and spill area as for launch_query_hits.
void launch_sweep_spheres(const SceneDev& sc, const float4* sweeps, uint32_t cull_mask, const float* inst_scale, HitRec* hits, uint32_t n, int32_t* ovf_stack,
                          uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s);
// the side of the reported triangle's plane every sphere's centre lies on at its contact (launch_closest_side's rule and word)
void launch_sweep_side(const SceneDev& sc, const float4* sweeps, const HitRec* hits, float4* attr, uint32_t n, hipStream_t s);
// rt_point_inside_device: the vote word of every point (16 bytes: p.xyz, ignored) over the crossing parities of the rays along the first
// n_dirs (1, 3 or 5) directions of RT_INSIDE_DIRS, counted as launch_query_hits counts them for the word 0 | cull_mask << 24
// (kernels_inside.inc), into words[n]; counts (optional): the n * n_dirs crossing counts, point-major, and then no early stop.  Chunk
// cursor, counters (counting) and spill area as for launch_query_hits.
void launch_point_inside(const SceneDev& sc, const float4* points, uint32_t cull_mask, uint32_t n_dirs, uint32_t* words, uint32_t* counts, uint32_t n,
                         int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s);
// rt_signed_distance_device: sets the sign bit of hits[i].t where bit 0 of words[i] is set and points[i] was a valid closest-point record
void launch_sign_distance(const float4* points, const uint32_t* words, HitRec* hits, uint32_t n, hipStream_t s);
// the side of the reported triangle's plane the segment's point P0 + params[i] (P1 - P0) lies on (launch_closest_side's rule and word)
void launch_segment_side(const SceneDev& sc, const float4* segs, const float* params, const HitRec* hits, float4* attr, uint32_t n, hipStream_t s);
// the side of the reported triangle's plane the query's point (P0 + qu (P1 - P0)) + qv (P2 - P0) lies on (launch_closest_side's rule and word)
void launch_triangle_side(const SceneDev& sc, const float4* tris, const float* params, const HitRec* hits, float4* attr, uint32_t n, hipStream_t s);
// rt_scene_triangles_device and the expansion in front of the two by-reference walks (kernels_refs.inc): the 48-byte record of every
// reference (16 bytes: inst, prim, against, r_max) into tris[3 n]: the world image of the source packet, r_max, inst and against in words
// 3, 7 and 11; nine quiet NaNs for an invalid reference.  n_vert_floats: the floats of sc.verts.
void launch_refs_expand(const SceneDev& sc, const void* refs, float4* tris, uint32_t n, uint64_t n_vert_floats, hipStream_t s);
// rt_overlap_*_device_list (kernels_list.inc; DESIGN.md §5 "Overlap lists").  The two thresholds of a row's length:
#ifndef RT_LIST_INSERT_MAX
#define RT_LIST_INSERT_MAX 64   /* a row of at most this many entries is kept sorted by insertion in the walk, as the capped calls keep theirs; a longer one goes to k_list_sort
                                   (measured: 4, 16, 32, 64, 128, 256 in profiles/overlap_lists.txt) */
#endif
#ifndef RT_LIST_LDS_TILE
#define RT_LIST_LDS_TILE 2048   /* entries k_list_sort sorts in LDS at once (16 KB: eight workgroups share a CU); a longer row is merged tile by tile through global memory */
#endif
// the n + 1 uint64 exclusive offsets of n uint32 counts (offsets[n]: their sum); sums: list_scan_tiles(n) words of scratch
uint32_t list_scan_tiles(uint32_t n);
void launch_list_scan(const uint32_t* counts, uint32_t n, unsigned long long* sums, unsigned long long* offsets, hipStream_t s);
// the fill walk behind launch_overlap's count-only walk (k == 0, counts) and the scan: row i, the whole candidate set in (inst, prim)
// order, at ids[offsets[i] .. offsets[i + 1]) if offsets[i + 1] <= capacity, then k_list_sort over the rows longer than
// RT_LIST_INSERT_MAX.  work: 1 + n words of scratch (the number of such rows, then their records).
void launch_overlap_list(OverlapShape shape, const SceneDev& sc, const float4* records, uint32_t cull_mask, const float* inst_scale, const unsigned long long* offsets,
                         void* ids, uint64_t capacity, uint32_t* work, uint32_t n, int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg,
                         hipStream_t s);
// rt_closest_instances_device, rt_overlap_instances_device (kernels_pairs.inc; DESIGN.md §5 "Instance pairs"): the by-reference triangle
// queries per record (16 bytes: inst, against, r_max, reserved), every triangle of the source instance a work item of the walk.
//   plan      items[n]: the work items of every record (0: invalid), offsets[n + 1] their starts (launch_list_scan; sums_scratch its
//             scratch), and the start values: keys[n] (nearest), or sums[n] and first_p[n] (overlap; first_p optional)
//   nearest   the shared-bound walk: keys[i] becomes bits(d2) << 32 | p of the record's nearest pair, its low word 0xFFFFFFFF on a miss
//   collide   the count-only walk: sums[i] the number of triangle pairs, first_p[i] the smallest source primitive with one (or
//             0xFFFFFFFF); any: sums[i] 0 or 1 and no first_p
//   refs      one rt_tri_ref per record from `word` (stride words apart: the keys' low words, or first_p): (inst, p, against, r_max or 0),
//             or (-1, -1, -1, r_max or 0); src_prims (optional): p or -1
//   first     (p, inst, prim, 0) from first_p and the capped by-reference call's rows of one
// max_items bounds the work items (their number stays on the device) and with it the grid; inst_scale, chunk cursor, counters
// (counting) and spill area as for launch_nearest; n_vert_floats as for launch_refs_expand.
void launch_pairs_plan(const SceneDev& sc, const void* irefs, uint32_t n, bool nearest, uint32_t* items, unsigned long long* sums_scratch, unsigned long long* offsets,
                       unsigned long long* keys, unsigned long long* sums, uint32_t* first_p, hipStream_t s);
void launch_pairs_nearest(const SceneDev& sc, const void* irefs, const unsigned long long* offsets, unsigned long long* keys, uint32_t cull_mask, const float* inst_scale,
                          uint32_t n, uint64_t max_items, uint64_t n_vert_floats, int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s);
void launch_pairs_collide(const SceneDev& sc, const void* irefs, const unsigned long long* offsets, unsigned long long* sums, uint32_t* first_p, bool any, uint32_t cull_mask,
                          const float* inst_scale, uint32_t n, uint64_t max_items, uint64_t n_vert_floats, int32_t* ovf_stack, uint32_t* counters, bool counting,
                          const LaunchCfg& cfg, hipStream_t s);
void launch_pairs_refs(const void* irefs, const uint32_t* word, uint32_t stride, uint32_t n, bool keep_radius, void* refs, int32_t* src_prims, hipStream_t s);
void launch_pairs_first(const uint32_t* first_p, const void* ids, uint32_t n, void* first4, hipStream_t s);
// rt_instance_pairs_device (kernels_ipairs.inc; DESIGN.md §5 "Instance broad phase"): the instances whose canonical boxes come within a
// record's margin of its source's, as rows of rt_inst_ref records in CSR form.
//   boxes   two float4 per instance of sc into `boxes` (the canonical box and its flags), from the n_meshes entries of the scene's device
//           mesh table (TlasMeshDev)
//   size    the count walk: counts[n], the rows' lengths (launch_list_scan makes the offsets of them)
//   fill    the fill walk: row i at pairs[offsets[i] .. offsets[i + 1]) if offsets[i + 1] <= capacity, in ascending `against`, then
//           k_ipairs_sort over the rows longer than RT_LIST_INSERT_MAX.  work: 1 + n words of scratch, as for launch_overlap_list
// inst_scale (launch_closest_scale fills it first: word 0 bounds every box's widening), chunk cursor, counters (counting: node visits
// and exact box tests) and spill area as for launch_overlap.
void launch_ipairs_boxes(const SceneDev& sc, const void* mesh_table, uint32_t n_meshes, float4* boxes, hipStream_t s);
void launch_ipairs_size(const SceneDev& sc, const void* irefs, const float4* boxes, const float* inst_scale, uint32_t cull_mask, bool above, uint32_t* counts, uint32_t n,
                        int32_t* ovf_stack, uint32_t* counters, bool counting, const LaunchCfg& cfg, hipStream_t s);
void launch_ipairs_fill(const SceneDev& sc, const void* irefs, const float4* boxes, const float* inst_scale, uint32_t cull_mask, bool above,
                        const unsigned long long* offsets, void* pairs, uint64_t capacity, uint32_t* work, uint32_t n, int32_t* ovf_stack, uint32_t* counters,
                        bool counting, const LaunchCfg& cfg, hipStream_t s);
// rt_shade_rays_device: k_ray_ingest replaces k_raygen for the caller's n rays (32 bytes each, o.xyz, w3, d.xyz, tmax; sample id = record
// index): sky colours of the rays that miss the TLAS and (0, 0, 0, 0) for invalid records into f.sample_color, the others into bounce queue 0
// (workgroup b appends to shard b % 8: f.shard_cap >= 256 * ceil(ray_ingest_block_count(n) / 8)).  f.counters must be zero.
uint32_t ray_ingest_block_count(uint32_t n);
void launch_ray_ingest(const SceneDev& sc, const FrameDev& f, const float4* rays, uint32_t n, hipStream_t s);
// k_resolve's per-pixel average for sample-major colours (sample i of point p at i * n_points + p) into out[n_points]
void launch_resolve_points(const float4* sample_color, float4* out, uint32_t n_points, uint32_t n_samples, hipStream_t s);

// de-interleave n_shards gathered compact shards (shard_stride_px pixels apart) into the width x height frame
void launch_assemble(const void* gathered, void* out, int width, int height, int band_rows, int n_shards, size_t shard_stride_px, bool rgba8, hipStream_t s);
int trace_threads_per_block();
// true in librt_mi355x_alt.so (-DRT_ALT_KERNELS): trace_variant 1 / 2, packet_trace, tile_blobs and shadow_beams exist; the product library
// has the one-lane BVH2 kernels only
bool alt_kernels_built();
// resident workgroups of k_tail per CU (occupancy query; <= 0 on failure)
int tail_blocks_per_cu();
// host-only sizing rules (rt_api.cpp)
size_t ovf_elems(int trace_blocks, int tail_blocks, uint32_t stride);
int tail_grid(int n_cu, int resident_blocks_per_cu, int live_slots);

}  // namespace rt
