"""ctypes mirror of include/rt_api.h (the C ABI of librt_mi355x.so)."""
import ctypes as C

import numpy as np

from . import _native

HIT_DTYPE = np.dtype([("t", np.float32), ("u", np.float32), ("v", np.float32), ("prim", np.int32), ("inst", np.int32)])
MESH_RANGE_DTYPE = np.dtype([("first_float", np.uint64), ("first_index", np.uint64), ("prim_count", np.uint32), ("reserved", np.uint32)])
INSTANCE_DTYPE = np.dtype([("transform", np.float32, 12), ("custom_index_and_mask", np.uint32), ("sbt_offset_and_flags", np.uint32), ("mesh", np.uint64)])
UNIFORMS_DTYPE = np.dtype([("position", np.float32, 4), ("right", np.float32, 4), ("up", np.float32, 4), ("forward", np.float32, 4),
                           ("light_position", np.float32, 3), ("light_intensity", np.float32),
                           ("max_bounce_count", np.uint32), ("samples_per_pixel", np.uint32),
                           ("center_object_type", np.uint32), ("orbiting_object_type", np.uint32),
                           ("orbiting_object_primitive_offset", np.uint32), ("orbiting_object_vertex_offset", np.uint32)])
MATERIAL_DTYPE = np.dtype([("ka", np.float32, 3), ("ns", np.float32), ("kd", np.float32, 3), ("ni", np.float32), ("ks", np.float32, 3), ("type", np.uint32)])
MATERIAL_TYPE_OF_INSTANCE = 0xFFFFFFFF
assert MATERIAL_DTYPE.itemsize == 48
# device records (csrc/rt_device.h, csrc/tlas_gpu.h) as rt_debug_snapshot / rt_debug_host_blas return them
NODEQ_DTYPE = np.dtype([("w", np.uint32, 6), ("child", np.int32, 2)])
TRI_PACKET_DTYPE = np.dtype([("v0", np.float32, 3), ("e1", np.float32, 3), ("e2", np.float32, 3), ("prim", np.uint32), ("pad", np.uint32, 2)])
INSTANCE_DEV_DTYPE = np.dtype([("w2o", np.float32, 12), ("o2w", np.float32, 12), ("blas_root", np.int32), ("mask", np.uint32), ("custom_index", np.int32),
                               ("first_float", np.uint32), ("first_index", np.uint32), ("blas_root4", np.int32), ("q_lo", np.float32, 3), ("q_scale", np.float32, 3),
                               ("type", np.uint32), ("cover_first", np.uint32), ("cover_count", np.uint32), ("prim_count", np.uint32)])
TLAS_MESH_DTYPE = np.dtype([("blas_root", np.int32), ("blas_root4", np.int32), ("first_float", np.uint32), ("first_index", np.uint32),
                            ("cover_first", np.uint32), ("cover_count", np.uint32), ("prim_count", np.uint32), ("built", np.uint32), ("levels", np.int32),
                            ("q_lo", np.float32, 3), ("q_scale", np.float32, 3), ("lo", np.float32, 3), ("hi", np.float32, 3)])
assert NODEQ_DTYPE.itemsize == 32 and TRI_PACKET_DTYPE.itemsize == 48 and INSTANCE_DEV_DTYPE.itemsize == 160 and TLAS_MESH_DTYPE.itemsize == 84
SNAPSHOT_INFO_WORDS = 20
assert INSTANCE_DTYPE.itemsize == 64 and UNIFORMS_DTYPE.itemsize == 104 and MESH_RANGE_DTYPE.itemsize == 24


class RtStats(C.Structure):
    _fields_ = [("rays_primary", C.c_uint64), ("rays_secondary", C.c_uint64), ("rays_shadow", C.c_uint64),
                ("node_visits", C.c_uint64), ("tri_tests", C.c_uint64), ("node_visits_shadow", C.c_uint64), ("tri_tests_shadow", C.c_uint64),
                ("diag", C.c_uint64 * 6), ("closest_rays", C.c_uint64),
                ("ms_frame", C.c_float), ("ms_raygen", C.c_float), ("ms_trace_closest", C.c_float), ("ms_trace_shadow", C.c_float),
                ("ms_shade", C.c_float), ("ms_resolve", C.c_float),
                ("launches_trace_closest", C.c_uint32), ("launches_total", C.c_uint32), ("timed_frames", C.c_uint32), ("ms_tail", C.c_float),
                ("bvh_node_bytes", C.c_uint32), ("bvh_tri_bytes", C.c_uint32), ("tail_faults", C.c_uint32), ("frames_rerendered", C.c_uint32),
                ("blob_tiles", C.c_uint64), ("blob_tiles_large", C.c_uint64), ("blob_tiles_refused", C.c_uint64), ("blob_nodes", C.c_uint64), ("blob_tris", C.c_uint64),
                ("tile_rays", C.c_uint64), ("tile_rays_handed_on", C.c_uint64), ("tile_diag", C.c_uint64 * 6), ("rays_shadow_untraced", C.c_uint64)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k in ("diag", "tile_diag") else getattr(self, k)) for k, _ in self._fields_}

    @property
    def rays_total(self):
        return self.rays_primary + self.rays_secondary + self.rays_shadow


# rt_intersect_device_flags (include/rt_api.h): gl_RayFlags*EXT values, VkGeometryInstanceFlagBitsKHR (high byte of sbt_offset_and_flags),
# and the hit kinds RayQuery.hit_kind reports
RAY_FLAG_NONE = 0x000
RAY_FLAG_OPAQUE = 0x001
RAY_FLAG_NO_OPAQUE = 0x002
RAY_FLAG_TERMINATE_ON_FIRST_HIT = 0x004
RAY_FLAG_SKIP_CLOSEST_HIT = 0x008
RAY_FLAG_CULL_BACK_FACING = 0x010
RAY_FLAG_CULL_FRONT_FACING = 0x020
RAY_FLAG_CULL_OPAQUE = 0x040
RAY_FLAG_CULL_NO_OPAQUE = 0x080
RAY_FLAG_SKIP_TRIANGLES = 0x100
RAY_FLAG_SKIP_AABBS = 0x200
INSTANCE_FLAG_FACING_CULL_DISABLE = 0x1
INSTANCE_FLAG_FLIP_FACING = 0x2
INSTANCE_FLAG_FORCE_OPAQUE = 0x4
INSTANCE_FLAG_FORCE_NO_OPAQUE = 0x8
HIT_KIND_FRONT_FACING = 0xFE
HIT_KIND_BACK_FACING = 0xFF
# rt_tri_ref (include/rt_api.h): a triangle of the scene as the query of overlap_scene_triangles* / closest_scene_triangle*
TRI_REF_DTYPE = np.dtype([("inst", np.int32), ("prim", np.int32), ("against", np.int32), ("r_max", np.float32)])
assert TRI_REF_DTYPE.itemsize == 16
REF_AGAINST_OTHERS = -1
# rt_inst_ref (include/rt_api.h): a whole instance as the query of closest_instances* / overlap_instances*
INST_REF_DTYPE = np.dtype([("inst", np.int32), ("against", np.int32), ("r_max", np.float32), ("reserved", np.uint32)])
assert INST_REF_DTYPE.itemsize == 16
OVERLAP_ANY = 0x1   # rt_overlap_boxes_device: occupancy (counts of 0 or 1)
INSTANCE_PAIRS_ABOVE = 0x1   # rt_instance_pairs_device: only candidates above the source instance
# rt_point_inside_device: the direction table (RT_INSIDE_DIRS of include/rt_api.h; rounded to binary32, not normalised)
INSIDE_DIRS = ((0.36, 0.48, 0.8), (-0.8, 0.36, -0.48), (0.48, -0.8, -0.36), (-0.6, -0.64, 0.48), (0.64, -0.48, 0.6))

EXPORTS = ["rt_create", "rt_create_frame_slot", "rt_destroy", "rt_upload_geometry", "rt_build_blas", "rt_set_instances", "rt_set_instances_device", "rt_refit_blas_device", "rt_set_materials", "rt_set_instance_types", "rt_set_uniforms", "rt_set_skybox",
           "rt_trace", "rt_trace_async", "rt_trace_wait", "rt_trace_shard", "rt_set_batch", "rt_trace_shard_batch", "rt_assemble_shards", "rt_shard_rows", "rt_synchronize", "rt_get_stats", "rt_set_timing", "rt_intersect",
           "rt_trace_counting", "rt_intersect_device", "rt_intersect_device_flags", "rt_intersect_device_hits", "rt_closest_point_device", "rt_closest_point", "rt_closest_point_device_hits", "rt_closest_point_hits", "rt_overlap_boxes_device", "rt_overlap_boxes", "rt_overlap_triangles_device", "rt_overlap_triangles", "rt_sweep_spheres_device", "rt_sweep_spheres", "rt_closest_segment_device", "rt_closest_segment", "rt_closest_triangle_device", "rt_closest_triangle", "rt_scene_triangles_device", "rt_overlap_scene_triangles_device", "rt_overlap_scene_triangles", "rt_overlap_boxes_device_list", "rt_overlap_boxes_list", "rt_overlap_triangles_device_list", "rt_overlap_triangles_list", "rt_overlap_scene_triangles_device_list", "rt_overlap_scene_triangles_list", "rt_closest_scene_triangle_device", "rt_closest_scene_triangle", "rt_closest_instances_device", "rt_closest_instances", "rt_overlap_instances_device", "rt_overlap_instances", "rt_instance_pairs_device", "rt_instance_pairs", "rt_point_inside_device", "rt_point_inside", "rt_signed_distance_device", "rt_shade_rays_device", "rt_set_param", "rt_debug_check_builders", "rt_debug_host_blas", "rt_debug_snapshot", "rt_debug_sizing", "rt_last_error", "rt_device_info", "rt_abi_version"]

_LIBS = {}


def lib(variant=None):
    """librt_mi355x.so, or librt_mi355x_<variant>.so (variant "alt": the build that also holds the traversal kernels which
    measured slower — k_packet, the quad/BVH4 kernel, 4-ary records, tile blobs, shadow beams; `make alt`).  RT_LIB_VARIANT names the default."""
    if variant not in _LIBS:
        L = _native.load_rt(variant)
        vp = C.c_void_p
        L.rt_create.argtypes = [C.POINTER(vp), C.c_int]
        L.rt_create_frame_slot.argtypes = [vp, C.POINTER(vp)]
        L.rt_destroy.argtypes = [vp]
        L.rt_destroy.restype = None
        L.rt_upload_geometry.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_int]
        L.rt_build_blas.argtypes = [vp, C.c_int]
        L.rt_set_instances.argtypes = [vp, vp, C.c_int, C.c_int]
        L.rt_set_instances_device.argtypes = [vp, vp, C.c_int, C.c_int, vp]
        L.rt_refit_blas_device.argtypes = [vp, C.c_int, vp, C.c_size_t, vp]
        L.rt_set_materials.argtypes = [vp, vp, C.c_int, vp, C.c_size_t]
        L.rt_set_instance_types.argtypes = [vp, vp, C.c_int]
        L.rt_set_uniforms.argtypes = [vp, vp]
        L.rt_set_skybox.argtypes = [vp, C.POINTER(vp), C.c_int, C.c_int]
        L.rt_trace.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(RtStats)]
        L.rt_trace_counting.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(RtStats)]
        L.rt_trace_async.argtypes = [vp, C.c_int, C.c_int]
        L.rt_trace_wait.argtypes = [vp, C.POINTER(vp), C.POINTER(RtStats)]
        L.rt_trace_shard.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp]
        L.rt_trace_shard_batch.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, C.c_size_t, vp]
        L.rt_set_batch.argtypes = [vp, C.c_int, vp, C.c_int, vp, C.c_int]
        L.rt_assemble_shards.argtypes = [vp, vp, C.c_int, C.c_size_t, C.c_int, C.c_int, C.c_int, vp, C.c_size_t, vp]
        L.rt_shard_rows.argtypes = [C.c_int] * 4
        L.rt_synchronize.argtypes = [vp]
        L.rt_get_stats.argtypes = [vp, C.POINTER(RtStats)]
        L.rt_set_timing.argtypes = [vp, C.c_int]
        L.rt_set_param.argtypes = [vp, C.c_char_p, C.c_int]
        L.rt_debug_check_builders.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp]
        L.rt_debug_sizing.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, vp]
        L.rt_debug_host_blas.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t, vp]
        L.rt_debug_snapshot.argtypes = [vp, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.rt_intersect.argtypes = [vp, C.c_size_t, vp, C.c_int, vp, C.c_int, C.POINTER(RtStats)]
        L.rt_intersect_device.argtypes = [vp, C.c_size_t, vp, C.c_int, vp, vp, vp]
        L.rt_intersect_device_flags.argtypes = [vp, C.c_size_t, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
        L.rt_intersect_device_hits.argtypes = [vp, C.c_size_t, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
        L.rt_closest_point_device.argtypes = [vp, C.c_size_t, vp, C.c_uint32, vp, vp, vp]
        L.rt_closest_point.argtypes = [vp, C.c_size_t, vp, C.c_uint32, vp, C.c_int, C.POINTER(RtStats)]
        L.rt_closest_point_device_hits.argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
        L.rt_closest_point_hits.argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_int, C.POINTER(RtStats)]
        L.rt_sweep_spheres_device.argtypes = [vp, C.c_size_t, vp, C.c_uint32, vp, vp, vp]
        L.rt_sweep_spheres.argtypes = [vp, C.c_size_t, vp, C.c_uint32, vp, C.c_int, C.POINTER(RtStats)]
        L.rt_closest_segment_device.argtypes = [vp, C.c_size_t, vp, C.c_uint32, vp, vp, vp, vp]
        L.rt_closest_segment.argtypes = [vp, C.c_size_t, vp, C.c_uint32, vp, vp, C.c_int, C.POINTER(RtStats)]
        L.rt_closest_triangle_device.argtypes = [vp, C.c_size_t, vp, C.c_uint32, vp, vp, vp, vp]
        L.rt_closest_triangle.argtypes = [vp, C.c_size_t, vp, C.c_uint32, vp, vp, C.c_int, C.POINTER(RtStats)]
        L.rt_point_inside_device.argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
        L.rt_point_inside.argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_int, C.POINTER(RtStats)]
        L.rt_signed_distance_device.argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp]
        L.rt_overlap_boxes_device.argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp]
        L.rt_overlap_boxes.argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, C.c_int, C.POINTER(RtStats)]
        L.rt_overlap_triangles_device.argtypes = L.rt_overlap_boxes_device.argtypes
        L.rt_overlap_triangles.argtypes = L.rt_overlap_boxes.argtypes
        L.rt_scene_triangles_device.argtypes = [vp, C.c_size_t, vp, vp, vp]
        L.rt_overlap_scene_triangles_device.argtypes = L.rt_overlap_boxes_device.argtypes
        L.rt_overlap_scene_triangles.argtypes = L.rt_overlap_boxes.argtypes
        for name in ("boxes", "triangles", "scene_triangles"):
            getattr(L, "rt_overlap_%s_device_list" % name).argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_size_t, vp]
            getattr(L, "rt_overlap_%s_list" % name).argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_size_t, C.c_int, C.POINTER(RtStats)]
        L.rt_closest_scene_triangle_device.argtypes = L.rt_closest_triangle_device.argtypes
        L.rt_closest_scene_triangle.argtypes = L.rt_closest_triangle.argtypes
        L.rt_closest_instances_device.argtypes = [vp, C.c_size_t, vp, C.c_uint32, vp, vp, vp, vp, vp]
        L.rt_closest_instances.argtypes = [vp, C.c_size_t, vp, C.c_uint32, vp, vp, vp, C.c_int, C.POINTER(RtStats)]
        L.rt_overlap_instances_device.argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, vp, vp]
        L.rt_overlap_instances.argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_int, C.POINTER(RtStats)]
        L.rt_instance_pairs_device.argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_size_t, vp]
        L.rt_instance_pairs.argtypes = [vp, C.c_size_t, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_size_t, C.c_int, C.POINTER(RtStats)]
        L.rt_shade_rays_device.argtypes = [vp, C.c_size_t, C.c_uint32, vp, vp, vp, vp]
        L.rt_last_error.argtypes = [vp]
        L.rt_last_error.restype = C.c_char_p
        L.rt_device_info.argtypes = [vp]
        L.rt_device_info.restype = C.c_char_p
        _LIBS[variant] = L
    return _LIBS[variant]


class RtError(RuntimeError):
    """Mirror of the reference's std::runtime_error("Vulkan API exception: return code N (fn)")
    (src/main.cpp:138-147)."""

    def __init__(self, code, fn, detail):
        super().__init__("RT API exception: return code %d (%s): %s" % (code, fn, detail))
        self.code = code


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class RtContext:
    """One context = one GPU (rt_create).  Methods map 1:1 onto the C ABI."""

    def __init__(self, device=0, _parent=None, variant=None):
        self.L = _parent.L if _parent is not None else lib(variant)
        h = C.c_void_p()
        if _parent is not None:
            rc = self.L.rt_create_frame_slot(_parent.h, C.byref(h))
        else:
            rc = self.L.rt_create(C.byref(h), device)
        if rc:
            raise RtError(rc, "rt_create_frame_slot" if _parent is not None else "rt_create", self.L.rt_last_error(None).decode())
        self.h = h
        self.device = _parent.device if _parent is not None else device

    def frame_slot(self):
        """rt_create_frame_slot: a context for one more frame in flight that shares this context's scene (geometry, BLAS,
        cube map) and owns its instances/TLAS, uniforms, queues and stream."""
        return RtContext(_parent=self)

    def _chk(self, rc, fn):
        if rc:
            raise RtError(rc, fn, self.L.rt_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.rt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_info(self):
        return self.L.rt_device_info(self.h).decode()

    def upload_geometry(self, verts6, idx, ranges, build=True):
        verts6 = np.ascontiguousarray(verts6, np.float32)
        idx = np.ascontiguousarray(idx, np.uint32)
        r = np.zeros(len(ranges), MESH_RANGE_DTYPE)
        for i, (ff, fi, pc) in enumerate(ranges):
            r[i] = (ff, fi, pc, 0)
        self._chk(self.L.rt_upload_geometry(self.h, _p(verts6), verts6.size, _p(idx), idx.size, _p(r), len(ranges)), "rt_upload_geometry")
        if build:
            for m in range(len(ranges)):
                self.build_blas(m)

    def build_blas(self, mesh):
        self._chk(self.L.rt_build_blas(self.h, mesh), "rt_build_blas")

    def set_instances(self, instances, update=False):
        inst = np.ascontiguousarray(instances, INSTANCE_DTYPE)
        self._chk(self.L.rt_set_instances(self.h, _p(inst), len(inst), int(update)), "rt_set_instances")

    def set_instances_device(self, t, update=False, stream=None):
        """rt_set_instances_device: the instance records are a contiguous torch tensor on this context's GPU holding n x 64 bytes
        (uint8 (n, 64), or any dtype whose byte size is a multiple of 64), read in the order of `stream` (default: the current
        torch stream of that device).  The TLAS is built (update=False) or refitted (update=True) on the GPU."""
        import torch
        if not isinstance(t, torch.Tensor):
            raise TypeError("set_instances_device takes a torch tensor, got %s" % type(t).__name__)
        if t.device.type != "cuda" or t.device.index != self.device:
            raise ValueError("instance tensor must live on cuda:%d (the context's GPU), not %s" % (self.device, t.device))
        if not t.is_contiguous():
            raise ValueError("instance tensor must be contiguous")
        nbytes = t.numel() * t.element_size()
        if t.dtype == torch.uint8 and t.dim() == 2 and t.shape[1] != INSTANCE_DTYPE.itemsize:
            raise ValueError("a uint8 instance tensor has shape (n, 64), got %s" % (tuple(t.shape),))
        if nbytes == 0 or nbytes % INSTANCE_DTYPE.itemsize:
            raise ValueError("instance tensor must hold n x 64 bytes (n >= 1), got %d bytes" % nbytes)
        if stream is None:
            stream = torch.cuda.current_stream(t.device)
        if stream.cuda_stream == 0:
            # torch's default stream is the null stream, which the C ABI reads as "the context's stream" (a non-blocking stream the
            # null stream does not order): the records must be complete before the library's copy starts
            stream.synchronize()
        self._chk(self.L.rt_set_instances_device(self.h, C.c_void_p(t.data_ptr()), nbytes // INSTANCE_DTYPE.itemsize, int(update),
                                                 C.c_void_p(stream.cuda_stream)), "rt_set_instances_device")

    def refit_blas_device(self, mesh, t, stream=None):
        """rt_refit_blas_device: mesh `mesh`'s new vertices, a contiguous float32 torch tensor on this context's GPU of shape (nv, 6) or
        (6 * nv,) in the upload layout (px py pz nx ny nz), covering the mesh's vertex span; read in the order of `stream` (default: the
        current torch stream of that device).  The BLAS is refitted on the GPU; every frame slot then needs its instances set again."""
        import torch
        if not isinstance(t, torch.Tensor):
            raise TypeError("refit_blas_device takes a torch tensor, got %s" % type(t).__name__)
        if t.device.type != "cuda" or t.device.index != self.device:
            raise ValueError("vertex tensor must live on cuda:%d (the context's GPU), not %s" % (self.device, t.device))
        if t.dtype != torch.float32:
            raise ValueError("vertex tensor must be float32, not %s" % t.dtype)
        if not t.is_contiguous():
            raise ValueError("vertex tensor must be contiguous")
        if not ((t.dim() == 2 and t.shape[1] == 6) or (t.dim() == 1 and t.shape[0] % 6 == 0)):
            raise ValueError("vertex tensor has shape (nv, 6) or (6 * nv,), got %s" % (tuple(t.shape),))
        if t.numel() == 0:
            raise ValueError("vertex tensor is empty")
        if stream is None:
            stream = torch.cuda.current_stream(t.device)
        if stream.cuda_stream == 0:
            # torch's default stream is the null stream, which the C ABI reads as "the context's stream" (a non-blocking stream the
            # null stream does not order): the vertices must be complete before the library's copy starts
            stream.synchronize()
        self._chk(self.L.rt_refit_blas_device(self.h, int(mesh), C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(stream.cuda_stream)),
                  "rt_refit_blas_device")

    def set_materials(self, table, prim_material=None):
        """row n4: MTL material table + material id of every triangle of the index buffer; table None/empty removes it"""
        if table is None or len(table) == 0:
            self._chk(self.L.rt_set_materials(self.h, None, 0, None, 0), "rt_set_materials")
            return
        t = np.ascontiguousarray(table, MATERIAL_DTYPE)
        pm = np.ascontiguousarray(prim_material, np.uint32)
        self._chk(self.L.rt_set_materials(self.h, _p(t), len(t), _p(pm), len(pm)), "rt_set_materials")

    def set_instance_types(self, types):
        t = np.ascontiguousarray(types if types is not None else [], np.uint32)
        self._chk(self.L.rt_set_instance_types(self.h, _p(t) if len(t) else None, len(t)), "rt_set_instance_types")

    def set_uniforms(self, uniforms):
        u = np.ascontiguousarray(uniforms, UNIFORMS_DTYPE).reshape(1)
        self._chk(self.L.rt_set_uniforms(self.h, _p(u)), "rt_set_uniforms")

    def set_skybox(self, faces):
        faces = [np.ascontiguousarray(f, np.uint8) for f in faces]
        assert len(faces) == 6
        h, w = faces[0].shape[:2]
        arr = (C.c_void_p * 6)(*[f.ctypes.data for f in faces])
        self._chk(self.L.rt_set_skybox(self.h, arr, w, h), "rt_set_skybox")

    def trace(self, W, H, counting=False):
        out = np.zeros((H, W, 4), np.uint8 if getattr(self, "_rgba8", False) else np.float32)
        st = RtStats()
        fn = self.L.rt_trace_counting if counting else self.L.rt_trace
        self._chk(fn(self.h, W, H, _p(out), C.byref(st)), "rt_trace")
        return out, st

    def shard_rows(self, H, band_rows, shard, n_shards):
        return self.L.rt_shard_rows(H, band_rows, shard, n_shards)

    def trace_async(self, W, H):
        """Enqueue a frame and its copy to the context's pinned host buffer; returns at once (one pending frame per context)."""
        self._chk(self.L.rt_trace_async(self.h, W, H), "rt_trace_async")
        self._async_shape = (H, W, 4)

    def trace_wait(self, copy=True):
        """Wait for the frame of trace_async; returns (pixels, stats).  With copy=False the array aliases the pinned
        buffer and is valid until the next trace_async on this context."""
        px = C.c_void_p()
        st = RtStats()
        self._chk(self.L.rt_trace_wait(self.h, C.byref(px), C.byref(st)), "rt_trace_wait")
        H, W, _ = self._async_shape
        ct = C.c_uint8 if getattr(self, "_rgba8", False) else C.c_float
        img = np.ctypeslib.as_array(C.cast(px, C.POINTER(ct)), shape=(H, W, 4))
        return (img.copy() if copy else img), st

    def trace_shard(self, W, H, band_rows, shard, n_shards, d_out_ptr, capacity_bytes, stream_ptr=None):
        self._chk(self.L.rt_trace_shard(self.h, W, H, band_rows, shard, n_shards, C.c_void_p(d_out_ptr), capacity_bytes,
                                        C.c_void_p(stream_ptr) if stream_ptr else None), "rt_trace_shard")

    def set_batch(self, instances, uniforms, update=False):
        """rt_set_batch: instances (K, n) records and K uniform blocks — K consecutive frames for one pass of the pipeline"""
        inst = np.ascontiguousarray(instances, INSTANCE_DTYPE)
        u = np.ascontiguousarray(uniforms, UNIFORMS_DTYPE).reshape(-1)
        K = len(u)
        inst = inst.reshape(K, -1)
        self._chk(self.L.rt_set_batch(self.h, K, _p(inst), inst.shape[1], _p(u), int(update)), "rt_set_batch")

    def trace_shard_batch(self, W, H, band_rows, shard, n_shards, d_out_ptr, capacity_bytes, stream_ptr=None, frame_stride_bytes=0):
        self._chk(self.L.rt_trace_shard_batch(self.h, W, H, band_rows, shard, n_shards, C.c_void_p(d_out_ptr), frame_stride_bytes, capacity_bytes,
                                              C.c_void_p(stream_ptr) if stream_ptr else None), "rt_trace_shard_batch")

    def assemble_shards(self, d_gathered_ptr, n_shards, shard_stride_bytes, W, H, band_rows, d_frame_ptr, capacity_bytes, stream_ptr=None):
        self._chk(self.L.rt_assemble_shards(self.h, C.c_void_p(d_gathered_ptr), n_shards, shard_stride_bytes, W, H, band_rows, C.c_void_p(d_frame_ptr),
                                            capacity_bytes, C.c_void_p(stream_ptr) if stream_ptr else None), "rt_assemble_shards")

    def synchronize(self):
        self._chk(self.L.rt_synchronize(self.h), "rt_synchronize")

    def stats(self):
        st = RtStats()
        self._chk(self.L.rt_get_stats(self.h, C.byref(st)), "rt_get_stats")
        return st

    def debug_snapshot(self):
        """rt_debug_snapshot (a test hook, not a product path): what this context's kernels read, copied to the host as numpy structured
        arrays in the device record layouts.  Returns a dict: the counts of the info call (n_blas_nodes, tlas_base, tlas_node_count,
        tlas_stride, batch_k, inst_per_frame), tlas_q_lo / tlas_q_scale (float32 (3,)), and the arrays blas_nodes, tlas_nodes (this
        context's region of its current parity, all frames of a batch), packets, instances, meshes, verts, idx, cover_boxes ((n, 6))."""
        info = np.zeros(SNAPSHOT_INFO_WORDS, np.uint64)
        self._chk(self.L.rt_debug_snapshot(self.h, 0, _p(info), info.nbytes, None), "rt_debug_snapshot")
        i = [int(x) for x in info]

        def item(what, n, dtype):
            a = np.zeros(n, dtype)
            got = C.c_size_t(0)
            self._chk(self.L.rt_debug_snapshot(self.h, what, _p(a) if n else _p(np.zeros(1, np.uint8)), a.nbytes, C.byref(got)), "rt_debug_snapshot")
            assert got.value == a.nbytes, (what, got.value, a.nbytes)
            return a

        bits = info[12:18].astype(np.uint32).view(np.float32)
        return {"n_blas_nodes": i[0], "tlas_base": i[1], "tlas_node_count": i[2], "tlas_stride": i[3], "batch_k": i[4], "inst_per_frame": i[7],
                "tlas_q_lo": bits[:3].copy(), "tlas_q_scale": bits[3:].copy(),
                "blas_nodes": item(1, i[0], NODEQ_DTYPE), "tlas_nodes": item(2, i[18], NODEQ_DTYPE), "packets": item(3, i[5], TRI_PACKET_DTYPE),
                "instances": item(4, i[6], INSTANCE_DEV_DTYPE), "meshes": item(5, i[8], TLAS_MESH_DTYPE), "verts": item(6, i[9], np.float32),
                "idx": item(7, i[10], np.uint32), "cover_boxes": item(8, 6 * i[11], np.float32).reshape(-1, 6)}

    def set_timing(self, on):
        self._chk(self.L.rt_set_timing(self.h, int(on)), "rt_set_timing")

    def set_param(self, name, value):
        self._chk(self.L.rt_set_param(self.h, name.encode(), int(value)), "rt_set_param")
        if name in ("output_rgba8", "output_bgra8"):
            self._rgba8 = bool(value)   # frames come back as uint8 (H, W, 4)

    def intersect(self, rays8, any_hit=False, counting=False):
        rays8 = np.ascontiguousarray(rays8, np.float32).reshape(-1, 8)
        out = np.zeros(len(rays8), HIT_DTYPE)
        st = RtStats()
        self._chk(self.L.rt_intersect(self.h, len(rays8), _p(rays8), int(any_hit), _p(out), int(counting), C.byref(st)), "rt_intersect")
        return out, st

    def intersect_device(self, rays, any_hit=False, attributes=False, stream=None, out=None):
        """rt_intersect_device: ray queries in device memory.  `rays` is a contiguous float32 torch tensor (n, 8) on this context's GPU
        (o.xyz, tmin, d.xyz, tmax per row), read in the order of `stream` (default: the current torch stream of that device); the
        results are written in that order too, and the call never waits on the host.  Returns a RayQuery of zero-copy views over one
        int32 (n, 5) hits buffer (rt_hit: t, u, v, prim, inst) and, with attributes=True (closest-hit queries only), one int32 (n, 8)
        attribute buffer (rt_hit_attr: position, object_index, normal, reserved).  out = (hits, attr) reuses such buffers."""
        def call(run, hits, attr):
            return self.L.rt_intersect_device(self.h, rays.shape[0], C.c_void_p(rays.data_ptr()), int(any_hit), C.c_void_p(hits.data_ptr()),
                                              C.c_void_p(attr.data_ptr()) if attr is not None else None, C.c_void_p(run.cuda_stream))
        hits, attr = self._device_query(rays, attributes, stream, out, (), call, "rt_intersect_device")
        return RayQuery(hits, attr)

    def intersect_device_flags(self, rays, ray_flags=0, cull_mask=0xFF, words=None, attributes=False, stream=None, out=None):
        """rt_intersect_device_flags: intersect_device with rayQueryInitializeEXT's rayFlags and cullMask, for the whole call and per ray.
        `words`, optional, is an int32 or uint32 (n,) tensor on the context's GPU: bits 0-9 ray flags, bits 24-31 the ray's cull mask
        (ray i traces with ray_flags | (word & 0x3FF) and cull_mask & (word >> 24)).  Attributes are allowed for first-hit rays too, and
        RayQuery.hit_kind holds the hit kind (HIT_KIND_FRONT_FACING / HIT_KIND_BACK_FACING, 0 on a miss).  See include/rt_api.h."""
        import torch
        n = rays.shape[0] if isinstance(rays, torch.Tensor) else 0
        if words is not None:
            if not isinstance(words, torch.Tensor):
                raise TypeError("words must be a torch tensor, got %s" % type(words).__name__)
            if words.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                raise ValueError("words must be int32 or uint32, not %s" % words.dtype)
            if words.device != getattr(rays, "device", None) or not words.is_contiguous() or tuple(words.shape) != (n,):
                raise ValueError("words must be a contiguous (n,) tensor on the rays' device")

        def call(run, hits, attr):
            return self.L.rt_intersect_device_flags(self.h, n, C.c_void_p(rays.data_ptr()), C.c_void_p(words.data_ptr()) if words is not None and n else None,
                                                    int(ray_flags) & 0xFFFFFFFF, int(cull_mask) & 0xFFFFFFFF, C.c_void_p(hits.data_ptr()),
                                                    C.c_void_p(attr.data_ptr()) if attr is not None else None, C.c_void_p(run.cuda_stream))
        hits, attr = self._device_query(rays, attributes, stream, out, (words,), call, "rt_intersect_device_flags")
        return RayQuery(hits, attr, hit_kind=True)

    def closest_point_device(self, points, cull_mask=0xFF, attributes=False, stream=None, out=None):
        """rt_closest_point_device: the nearest surface point of every query point.  `points` is a contiguous float32 torch tensor (n, 4)
        on this context's GPU (x, y, z, r_max per row: a world-space point and a search radius, inf allowed), read in the order of
        `stream` like intersect_device's rays.  Returns a RayQuery: t the distance, u / v the nearest point's barycentrics, prim / inst the
        triangle (a miss: t = r_max, prim = inst = -1); with attributes=True position is the nearest point, normal the shading normal
        there and hit_kind the side of the triangle's plane the point lies on.  out = (hits, attr) reuses buffers.  See include/rt_api.h."""
        def call(run, hits, attr):
            return self.L.rt_closest_point_device(self.h, points.shape[0], C.c_void_p(points.data_ptr()), int(cull_mask) & 0xFFFFFFFF, C.c_void_p(hits.data_ptr()),
                                                  C.c_void_p(attr.data_ptr()) if attr is not None else None, C.c_void_p(run.cuda_stream))
        hits, attr = self._device_query(points, attributes, stream, out, (), call, "rt_closest_point_device", cols=4)
        return RayQuery(hits, attr, hit_kind=True)

    def closest_point(self, points4, cull_mask=0xFF, counting=False):
        """rt_closest_point: the blocking host form -> (HIT_DTYPE records, RtStats; with counting its node_visits / tri_tests are filled)"""
        points4 = np.ascontiguousarray(points4, np.float32).reshape(-1, 4)
        out = np.zeros(len(points4), HIT_DTYPE)
        st = RtStats()
        self._chk(self.L.rt_closest_point(self.h, len(points4), _p(points4), int(cull_mask) & 0xFFFFFFFF, _p(out), int(counting), C.byref(st)), "rt_closest_point")
        return out, st

    def sweep_spheres_device(self, sweeps, cull_mask=0xFF, attributes=False, stream=None, out=None):
        """rt_sweep_spheres_device: the first contact of every moving sphere.  `sweeps` is a contiguous float32 torch tensor (n, 8) on this
        context's GPU (o.xyz, r, d.xyz, tmax per row: the sphere of radius r with its centre at o + t d, t in [0, tmax], inf allowed),
        read in the order of `stream` like intersect_device's rays.  Returns a RayQuery: t the contact time in units of d, u / v the
        contact point's barycentrics, prim / inst the triangle (a miss: t = tmax, prim = inst = -1); with attributes=True position is
        the contact point, normal the shading normal there and hit_kind the side of the triangle's plane the centre lies on at the
        contact.  out = (hits, attr) reuses buffers.  See include/rt_api.h."""
        def call(run, hits, attr):
            return self.L.rt_sweep_spheres_device(self.h, sweeps.shape[0], C.c_void_p(sweeps.data_ptr()), int(cull_mask) & 0xFFFFFFFF, C.c_void_p(hits.data_ptr()),
                                                  C.c_void_p(attr.data_ptr()) if attr is not None else None, C.c_void_p(run.cuda_stream))
        self._check_rays(sweeps, "sweep_spheres_device", 8, "sweep")
        hits, attr = self._device_query(sweeps, attributes, stream, out, (), call, "rt_sweep_spheres_device")
        return RayQuery(hits, attr, hit_kind=True)

    def sweep_spheres(self, sweeps8, cull_mask=0xFF, counting=False):
        """rt_sweep_spheres: the blocking host form -> (HIT_DTYPE records, RtStats; with counting its node_visits / tri_tests are filled)"""
        sweeps8 = np.ascontiguousarray(sweeps8, np.float32).reshape(-1, 8)
        out = np.zeros(len(sweeps8), HIT_DTYPE)
        st = RtStats()
        self._chk(self.L.rt_sweep_spheres(self.h, len(sweeps8), _p(sweeps8), int(cull_mask) & 0xFFFFFFFF, _p(out), int(counting), C.byref(st)), "rt_sweep_spheres")
        return out, st

    def closest_segment_device(self, segments, cull_mask=0xFF, attributes=False, params=False, stream=None, out=None):
        """rt_closest_segment_device: the nearest pair of every segment and the scene's surface.  `segments` is a contiguous float32 torch
        tensor (n, 8) on this context's GPU (P0.xyz, r_max, P1.xyz, ignored per row: the closed world-space segment P0..P1 and a search
        radius, inf allowed; capsule_records packs it), read in the order of `stream` like intersect_device's rays.  Returns a RayQuery:
        t the distance, u / v the barycentrics of the triangle's point of the nearest pair, prim / inst the triangle (a miss: t = r_max,
        prim = inst = -1); with attributes=True position is that surface point, normal the shading normal there and hit_kind the side of
        the triangle's plane the segment's point lies on; with params=True its `s` is a float32 (n,) tensor, the segment's point of the
        pair being P0 + s (P1 - P0) (0 on a miss), else None.  out = (hits, attr) or (hits, attr, s) reuses buffers.  A pierced
        triangle reports a rounding residue, not an exact 0.  See include/rt_api.h."""
        import torch
        self._check_rays(segments, "closest_segment_device", 8, "segment")
        n = segments.shape[0]
        s = None
        if out is not None and len(out) == 3:
            s, out = out[2], tuple(out[:2])
            if params and (s is None or s.dtype != torch.float32 or tuple(s.shape) != (n,) or not s.is_contiguous() or s.device != segments.device):
                raise ValueError("out s must be a contiguous float32 (n,) tensor on the segments' device")
        if not params:
            s = None
        elif s is None:
            s = torch.empty((n,), dtype=torch.float32, device=segments.device)

        def call(run, hits, attr):
            if s is not None:
                s.record_stream(run)
            return self.L.rt_closest_segment_device(self.h, n, C.c_void_p(segments.data_ptr()), int(cull_mask) & 0xFFFFFFFF, C.c_void_p(hits.data_ptr()),
                                                    C.c_void_p(attr.data_ptr()) if attr is not None else None,
                                                    C.c_void_p(s.data_ptr()) if s is not None else None, C.c_void_p(run.cuda_stream))
        hits, attr = self._device_query(segments, attributes, stream, out, (), call, "rt_closest_segment_device")
        res = RayQuery(hits, attr, hit_kind=True)
        res.s = s
        return res

    def closest_segment(self, segs8, cull_mask=0xFF, params=False, counting=False):
        """rt_closest_segment: the blocking host form -> (HIT_DTYPE records, RtStats; with counting its node_visits / tri_tests are
        filled), or with params=True (records, s float32 (n,), RtStats)"""
        segs8 = np.ascontiguousarray(segs8, np.float32).reshape(-1, 8)
        out = np.zeros(len(segs8), HIT_DTYPE)
        s = np.zeros(len(segs8), np.float32) if params else None
        st = RtStats()
        self._chk(self.L.rt_closest_segment(self.h, len(segs8), _p(segs8), int(cull_mask) & 0xFFFFFFFF, _p(out), _p(s) if s is not None else None,
                                            int(counting), C.byref(st)), "rt_closest_segment")
        return (out, s, st) if params else (out, st)

    def closest_triangle_device(self, tris, cull_mask=0xFF, attributes=False, params=False, stream=None, out=None):
        """rt_closest_triangle_device: the nearest pair of every query triangle and the scene's surface.  `tris` is
        overlap_triangles_device's tensor, a contiguous float32 (n, 12) on this context's GPU (P0.xyz, r_max, P1.xyz, ignored, P2.xyz,
        ignored per row: a closed world-space triangle and a search radius, inf allowed; triangle_records(..., r_max=) packs it), read
        in the order of `stream` like intersect_device's rays.  Returns a RayQuery: t the distance, u / v the barycentrics of the scene
        triangle's point of the nearest pair, prim / inst the scene triangle (a miss: t = r_max, prim = inst = -1); with
        attributes=True position is that surface point, normal the shading normal there and hit_kind the side of the scene triangle's
        plane the query's point lies on; with params=True its `quv` is a float32 (n, 2) tensor, the query's point of the pair being
        P0 + qu (P1 - P0) + qv (P2 - P0) (0, 0 on a miss), else None.  out = (hits, attr) or (hits, attr, quv) reuses buffers.  A
        scene triangle that cuts the query reports a rounding residue, not an exact 0.  See include/rt_api.h."""
        import torch
        self._check_rays(tris, "closest_triangle_device", 12, "triangle")
        n = tris.shape[0]
        quv = None
        if out is not None and len(out) == 3:
            quv, out = out[2], tuple(out[:2])
            if params and (quv is None or quv.dtype != torch.float32 or tuple(quv.shape) != (n, 2) or not quv.is_contiguous() or quv.device != tris.device):
                raise ValueError("out quv must be a contiguous float32 (n, 2) tensor on the triangles' device")
        if not params:
            quv = None
        elif quv is None:
            quv = torch.empty((n, 2), dtype=torch.float32, device=tris.device)

        def call(run, hits, attr):
            if quv is not None:
                quv.record_stream(run)
            return self.L.rt_closest_triangle_device(self.h, n, C.c_void_p(tris.data_ptr()), int(cull_mask) & 0xFFFFFFFF, C.c_void_p(hits.data_ptr()),
                                                     C.c_void_p(attr.data_ptr()) if attr is not None else None,
                                                     C.c_void_p(quv.data_ptr()) if quv is not None else None, C.c_void_p(run.cuda_stream))
        hits, attr = self._device_query(tris, attributes, stream, out, (), call, "rt_closest_triangle_device", cols=12, checked=True)
        res = RayQuery(hits, attr, hit_kind=True)
        res.quv = quv
        return res

    def closest_triangle(self, tris12, cull_mask=0xFF, params=False, counting=False):
        """rt_closest_triangle: the blocking host form -> (HIT_DTYPE records, RtStats; with counting its node_visits / tri_tests are
        filled), or with params=True (records, (qu, qv) float32 (n, 2), RtStats)"""
        tris12 = np.ascontiguousarray(tris12, np.float32).reshape(-1, 12)
        out = np.zeros(len(tris12), HIT_DTYPE)
        quv = np.zeros((len(tris12), 2), np.float32) if params else None
        st = RtStats()
        self._chk(self.L.rt_closest_triangle(self.h, len(tris12), _p(tris12), int(cull_mask) & 0xFFFFFFFF, _p(out), _p(quv) if quv is not None else None,
                                             int(counting), C.byref(st)), "rt_closest_triangle")
        return (out, quv, st) if params else (out, st)

    def point_inside_device(self, points, n_dirs=3, cull_mask=0xFF, counts=False, stream=None, out=None):
        """rt_point_inside_device: is every point enclosed by the scene's surfaces?  `points` is closest_point_device's tensor, a contiguous
        float32 (n, 4) on this context's GPU (x, y, z, ignored per row), read in the order of `stream` like intersect_device's rays.  The
        answer is the majority of the crossing parities of the rays from the point along the first n_dirs (1, 3 or 5) rows of INSIDE_DIRS.
        Returns a PointsInside: word, int32 (n,) (bit 0: inside; bits 8-15: odd votes; bits 16-23: directions taken), inside, its bit 0 as
        a bool tensor, and with counts=True count, int32 (n, n_dirs), the crossings of every direction (then every direction is taken).
        out = (word, count) reuses such buffers (None where not asked for).  See include/rt_api.h."""
        import torch
        self._check_rays(points, "point_inside_device", 4, "point")
        k = int(n_dirs)
        if k not in (1, 3, 5):
            raise ValueError("n_dirs must be 1, 3 or 5, got %d" % k)
        n = points.shape[0]
        cur = torch.cuda.current_stream(points.device)
        if stream is None:
            stream = cur
        shapes = ((n,), (n, k) if counts else None)
        if out is None:
            bufs = [torch.empty(sh, dtype=torch.int32, device=points.device) if sh is not None else None for sh in shapes]
            if stream != cur:   # (allocated for the current stream, written on `stream`)
                for t in bufs:
                    if t is not None:
                        t.record_stream(stream)
        else:
            bufs = list(out)
            for i, (t, sh, what) in enumerate(zip(bufs, shapes, ("words", "counts"))):
                if sh is None:
                    bufs[i] = None
                elif t is None or t.dtype != torch.int32 or tuple(t.shape) != sh or not t.is_contiguous() or t.device != points.device:
                    raise ValueError("out %s must be a contiguous int32 %s tensor on the points' device" % (what, sh))
        word, count = bufs

        def call(run):
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
            return self.L.rt_point_inside_device(self.h, n, ptr(points), int(cull_mask) & 0xFFFFFFFF, k, ptr(word), ptr(count), C.c_void_p(run.cuda_stream))
        if n:
            self._on_stream(stream, (points, word, count), call, "rt_point_inside_device")
        return PointsInside(word, count)

    def point_inside(self, points4, n_dirs=3, cull_mask=0xFF, counts=False, counting=False):
        """rt_point_inside: the blocking host form -> (words uint32 (n,), counts uint32 (n, n_dirs) or None, RtStats; with counting its
        node_visits / tri_tests are filled)"""
        points4 = np.ascontiguousarray(points4, np.float32).reshape(-1, 4)
        n, k = len(points4), int(n_dirs)
        word = np.zeros(n, np.uint32)
        cnt = np.zeros((n, max(k, 0)), np.uint32) if counts else None
        st = RtStats()
        self._chk(self.L.rt_point_inside(self.h, n, _p(points4), int(cull_mask) & 0xFFFFFFFF, k & 0xFFFFFFFF, _p(word),
                                         _p(cnt) if cnt is not None else None, int(counting), C.byref(st)), "rt_point_inside")
        return word, cnt, st

    def signed_distance_device(self, points, n_dirs=3, cull_mask=0xFF, attributes=False, stream=None, out=None, words=False):
        """rt_signed_distance_device: closest_point_device and point_inside_device in one call.  Returns closest_point_device's RayQuery
        with the sign bit of t set for the points inside (a miss inside: -r_max; t = 0 inside: -0.0); everything else is byte for byte
        closest_point_device's.  out = (hits, attr) reuses buffers.  With words=True the result's `word` is point_inside_device's int32
        (n,) vote word of every point (early stop).  See include/rt_api.h."""
        import torch
        k = int(n_dirs)
        if k not in (1, 3, 5):
            raise ValueError("n_dirs must be 1, 3 or 5, got %d" % k)
        word = None

        def call(run, hits, attr):
            if word is not None:
                word.record_stream(run)
            return self.L.rt_signed_distance_device(self.h, points.shape[0], C.c_void_p(points.data_ptr()), int(cull_mask) & 0xFFFFFFFF, k, C.c_void_p(hits.data_ptr()),
                                                    C.c_void_p(attr.data_ptr()) if attr is not None else None,
                                                    C.c_void_p(word.data_ptr()) if word is not None else None, C.c_void_p(run.cuda_stream))
        self._check_rays(points, "signed_distance_device", 4, "point")
        if words:
            word = torch.empty((points.shape[0],), dtype=torch.int32, device=points.device)
        hits, attr = self._device_query(points, attributes, stream, out, (), call, "rt_signed_distance_device", cols=4)
        res = RayQuery(hits, attr, hit_kind=True)
        res.word = word
        return res

    def overlap_boxes_device(self, boxes, max_ids=0, cull_mask=0xFF, any=False, counts=True, stream=None, out=None):
        """rt_overlap_boxes_device: the triangles that touch every query box.  `boxes` is a contiguous float32 torch tensor (n, 8) on this
        context's GPU (lo.xyz, ignored, hi.xyz, ignored per row: a closed world-space box), read in the order of `stream` like
        intersect_device's rays.  Returns a BoxOverlaps: count, int32 (n,), the number of triangles the canonical predicate does not
        separate from the box (with counts=True; required when max_ids is 0), and ids, int32 (n, max_ids, 2), the max_ids smallest
        (inst, prim) of them in ascending order, (-1, -1) past the last.  counts=False lets the walk stop once a row is full.  any=True
        answers occupancy (max_ids 0): count is 0 or 1.  out = (ids, count) reuses such buffers (None where not asked for).  See
        include/rt_api.h."""
        return self._overlap_device(boxes, "overlap_boxes", 8, "box", "boxes", max_ids, cull_mask, any, counts, stream, out)

    def _overlap_device(self, boxes, name, cols, noun, nouns, max_ids, cull_mask, any, counts, stream, out, int32=False):
        """overlap_boxes_device, overlap_triangles_device and overlap_scene_triangles_device (int32 records): the checks, the buffers and
        the call rt_<name>_device on `stream`"""
        import torch
        self._check_rays(boxes, name + "_device", cols, noun, int32)
        fn = getattr(self.L, "rt_%s_device" % name)
        k = int(max_ids)
        if not 0 <= k <= 16:
            raise ValueError("max_ids must be 0..16, got %d" % k)
        if k == 0 and not counts:
            raise ValueError("max_ids 0 counts only: counts=True")
        if any and k:
            raise ValueError("any=True answers occupancy: max_ids must be 0")
        n = boxes.shape[0]
        cur = torch.cuda.current_stream(boxes.device)
        if stream is None:
            stream = cur
        shapes = ((n, k, 2) if k else None, (n,) if counts else None)
        if out is None:
            bufs = [torch.empty(sh, dtype=torch.int32, device=boxes.device) if sh is not None else None for sh in shapes]
            if stream != cur:   # (allocated for the current stream, written on `stream`)
                for t in bufs:
                    if t is not None:
                        t.record_stream(stream)
        else:
            bufs = list(out)
            for i, (t, sh, what) in enumerate(zip(bufs, shapes, ("ids", "counts"))):
                if sh is None:
                    bufs[i] = None
                elif t is None or t.dtype != torch.int32 or tuple(t.shape) != sh or not t.is_contiguous() or t.device != boxes.device:
                    raise ValueError("out %s must be a contiguous int32 %s tensor on the %s' device" % (what, sh, nouns))
        ids, count = bufs

        def call(run):
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
            return fn(self.h, n, ptr(boxes), int(cull_mask) & 0xFFFFFFFF, OVERLAP_ANY if any else 0, k, ptr(ids), ptr(count), C.c_void_p(run.cuda_stream))
        if n:
            self._on_stream(stream, (boxes, ids, count), call, "rt_%s_device" % name)
        return BoxOverlaps(ids, count)

    def overlap_boxes(self, boxes8, max_ids=0, cull_mask=0xFF, any=False, counts=True, counting=False):
        """rt_overlap_boxes: the blocking host form -> (counts uint32 (n,) or None, ids int32 (n, max_ids, 2) or None, RtStats; with
        counting its node_visits / tri_tests are filled)"""
        boxes8 = np.ascontiguousarray(boxes8, np.float32).reshape(-1, 8)
        n, k = len(boxes8), int(max_ids)
        cnt = np.zeros(n, np.uint32) if counts else None
        ids = np.zeros((n, k, 2), np.int32) if k else None
        st = RtStats()
        self._chk(self.L.rt_overlap_boxes(self.h, n, _p(boxes8), int(cull_mask) & 0xFFFFFFFF, OVERLAP_ANY if any else 0, k & 0xFFFFFFFF,
                                          _p(ids) if ids is not None else None, _p(cnt) if cnt is not None else None, int(counting), C.byref(st)),
                  "rt_overlap_boxes")
        return cnt, ids, st

    def overlap_triangles_device(self, tris, max_ids=0, cull_mask=0xFF, any=False, counts=True, stream=None, out=None):
        """rt_overlap_triangles_device: the triangles of the scene that cut or touch every query triangle.  `tris` is a contiguous float32
        torch tensor (n, 12) on this context's GPU (P0.xyz, ignored, P1.xyz, ignored, P2.xyz, ignored per row: a closed world-space
        triangle; triangle_records builds such rows from a mesh), read in the order of `stream`.  Every other argument and the BoxOverlaps
        result as for overlap_boxes_device.  For triangles of the scene itself see overlap_scene_triangles_device; for others cull_mask is how an
        instance the queries came from is left out.  See include/rt_api.h."""
        return self._overlap_device(tris, "overlap_triangles", 12, "triangle", "triangles", max_ids, cull_mask, any, counts, stream, out)

    def overlap_triangles(self, tris12, max_ids=0, cull_mask=0xFF, any=False, counts=True, counting=False):
        """rt_overlap_triangles: the blocking host form -> (counts uint32 (n,) or None, ids int32 (n, max_ids, 2) or None, RtStats; with
        counting its node_visits / tri_tests are filled)"""
        tris12 = np.ascontiguousarray(tris12, np.float32).reshape(-1, 12)
        n, k = len(tris12), int(max_ids)
        cnt = np.zeros(n, np.uint32) if counts else None
        ids = np.zeros((n, k, 2), np.int32) if k else None
        st = RtStats()
        self._chk(self.L.rt_overlap_triangles(self.h, n, _p(tris12), int(cull_mask) & 0xFFFFFFFF, OVERLAP_ANY if any else 0, k & 0xFFFFFFFF,
                                              _p(ids) if ids is not None else None, _p(cnt) if cnt is not None else None, int(counting), C.byref(st)),
                  "rt_overlap_triangles")
        return cnt, ids, st

    def scene_triangles_device(self, refs, stream=None, out=None):
        """rt_scene_triangles_device: the world triangles of (inst, prim) references.  `refs` is a contiguous int32 torch tensor (n, 4) on
        this context's GPU (inst, prim, against, the bits of r_max per row; triangle_refs packs it), read in the order of `stream`.
        Returns a float32 (n, 12) tensor in overlap_triangles_device's layout: P0.xyz, r_max, P1.xyz, the bits of inst, P2.xyz, the bits
        of against; an invalid reference has nine NaNs.  out reuses such a tensor.  See include/rt_api.h."""
        import torch
        self._check_rays(refs, "scene_triangles_device", 4, "reference", True)
        n = refs.shape[0]
        cur = torch.cuda.current_stream(refs.device)
        if stream is None:
            stream = cur
        if out is None:
            out = torch.empty((n, 12), dtype=torch.float32, device=refs.device)
            if stream != cur:   # (allocated for the current stream, written on `stream`)
                out.record_stream(stream)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or tuple(out.shape) != (n, 12) or not out.is_contiguous() or out.device != refs.device:
            raise ValueError("out must be a contiguous float32 (n, 12) tensor on the references' device")

        def call(run):
            return self.L.rt_scene_triangles_device(self.h, n, C.c_void_p(refs.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(run.cuda_stream))
        if n:
            self._on_stream(stream, (refs, out), call, "rt_scene_triangles_device")
        return out

    def overlap_scene_triangles_device(self, refs, max_ids=0, cull_mask=0xFF, any=False, counts=True, stream=None, out=None):
        """rt_overlap_scene_triangles_device: overlap_triangles_device asked about triangles of the scene itself.  `refs` is
        scene_triangles_device's tensor (triangle_refs packs it): against = -1 takes candidates from every instance but the source's,
        against >= 0 from that instance only.  Every other argument and the BoxOverlaps result as for overlap_triangles_device.  See
        include/rt_api.h."""
        return self._overlap_device(refs, "overlap_scene_triangles", 4, "reference", "references", max_ids, cull_mask, any, counts, stream, out, int32=True)

    def overlap_scene_triangles(self, refs, max_ids=0, cull_mask=0xFF, any=False, counts=True, counting=False):
        """rt_overlap_scene_triangles: the blocking host form (refs: TRI_REF_DTYPE records or (n, 4) int32 rows) -> (counts uint32 (n,) or
        None, ids int32 (n, max_ids, 2) or None, RtStats; with counting its node_visits / tri_tests are filled)"""
        refs = _host_refs(refs)
        n, k = len(refs), int(max_ids)
        cnt = np.zeros(n, np.uint32) if counts else None
        ids = np.zeros((n, k, 2), np.int32) if k else None
        st = RtStats()
        self._chk(self.L.rt_overlap_scene_triangles(self.h, n, _p(refs), int(cull_mask) & 0xFFFFFFFF, OVERLAP_ANY if any else 0, k & 0xFFFFFFFF,
                                                    _p(ids) if ids is not None else None, _p(cnt) if cnt is not None else None, int(counting), C.byref(st)),
                  "rt_overlap_scene_triangles")
        return cnt, ids, st

    def overlap_boxes_device_list(self, boxes, capacity=None, cull_mask=0xFF, stream=None, out=None):
        """rt_overlap_boxes_device_list: every triangle that touches every query box, in CSR form.  `boxes` as for overlap_boxes_device.
        Returns an OverlapList: offsets, int64 (n + 1,), the row starts (offsets[n]: the total T, always complete); ids, int32
        (capacity, 2), row i the whole candidate set of box i in ascending (inst, prim) order at ids[offsets[i]:offsets[i + 1]], written
        if and only if offsets[i + 1] <= capacity (capacity 0: ids is None, offsets only); total, a 0-d view of offsets[n] (reading it
        is the caller's synchronisation).  out = (offsets, ids) reuses such buffers, and capacity then defaults to the rows of ids.
        With capacity=None and no out the wrapper makes an offsets-only call, reads the total ON THE HOST (a synchronisation),
        allocates exactly and calls again: three walks instead of two.  A loop is better served by a persistent ids buffer passed
        through out, and a second call with a larger one when total exceeds it.  See include/rt_api.h."""
        return self._overlap_list_device(boxes, "overlap_boxes", 8, "box", capacity, cull_mask, stream, out)

    def overlap_triangles_device_list(self, tris, capacity=None, cull_mask=0xFF, stream=None, out=None):
        """rt_overlap_triangles_device_list: every triangle of the scene that cuts or touches every query triangle (`tris` as for
        overlap_triangles_device), as overlap_boxes_device_list returns them."""
        return self._overlap_list_device(tris, "overlap_triangles", 12, "triangle", capacity, cull_mask, stream, out)

    def overlap_scene_triangles_device_list(self, refs, capacity=None, cull_mask=0xFF, stream=None, out=None):
        """rt_overlap_scene_triangles_device_list: overlap_triangles_device_list asked about triangles of the scene itself (`refs` as
        for overlap_scene_triangles_device)."""
        return self._overlap_list_device(refs, "overlap_scene_triangles", 4, "reference", capacity, cull_mask, stream, out, int32=True)

    def _overlap_list_device(self, records, name, cols, noun, capacity, cull_mask, stream, out, int32=False, width=2, flags=0, suffix="_device_list"):
        """the three *_device_list calls and instance_pairs_device (rows of `width` int32, `flags`): the checks, the buffers and
        rt_<name><suffix> on `stream`"""
        import torch
        self._check_rays(records, name + suffix, cols, noun, int32)
        fn = getattr(self.L, "rt_%s%s" % (name, suffix))
        n = records.shape[0]
        cur = torch.cuda.current_stream(records.device)
        if stream is None:
            stream = cur
        fresh = []
        if out is None:
            offsets = torch.zeros(n + 1, dtype=torch.int64, device=records.device) if n == 0 else torch.empty(n + 1, dtype=torch.int64, device=records.device)
            ids = None
            fresh.append(offsets)
        else:
            offsets, ids = out
            if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or tuple(offsets.shape) != (n + 1,) or not offsets.is_contiguous() or offsets.device != records.device:
                raise ValueError("out offsets must be a contiguous int64 (n + 1,) tensor on the records' device")
            if ids is not None and (not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 2 or ids.shape[1] != width or not ids.is_contiguous() or ids.device != records.device):
                raise ValueError("out rows must be a contiguous int32 (capacity, %d) tensor on the records' device, or None" % width)
            if capacity is None:
                capacity = ids.shape[0] if ids is not None else 0
            elif int(capacity) != (ids.shape[0] if ids is not None else 0):
                raise ValueError("capacity must be the rows of out ids")
        if stream != cur:   # (allocated for the current stream, written on `stream`)
            for t in fresh:
                t.record_stream(stream)

        def run_call(ids_t, cap):
            def call(run):
                return fn(self.h, n, C.c_void_p(records.data_ptr()), int(cull_mask) & 0xFFFFFFFF, flags, C.c_void_p(offsets.data_ptr()),
                          C.c_void_p(ids_t.data_ptr()) if ids_t is not None else None, cap, C.c_void_p(run.cuda_stream))
            if n:
                self._on_stream(stream, (records, offsets, ids_t), call, "rt_%s%s" % (name, suffix))
        if capacity is None:   # the offsets first, the total read on the host, then the exact allocation
            run_call(None, 0)
            if n:
                stream.synchronize()
            capacity = int(offsets[n].item()) if n else 0
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("capacity must not be negative")
        if capacity and ids is None:
            ids = torch.empty((capacity, width), dtype=torch.int32, device=records.device)
            if stream != cur:
                ids.record_stream(stream)
        run_call(ids if capacity else None, capacity)
        return OverlapList(offsets, ids if capacity else None)

    def _overlap_list_host(self, records, name, capacity, cull_mask, counting):
        """the three blocking *_list forms -> (offsets uint64 (n + 1,), ids int32 (capacity, 2) or None, RtStats); capacity=None: an
        offsets-only call first, then one with exactly the total"""
        fn = getattr(self.L, "rt_%s_list" % name)
        n = len(records)
        offsets = np.zeros(n + 1, np.uint64)
        st = RtStats()

        def call(ids, cap):
            self._chk(fn(self.h, n, _p(records), int(cull_mask) & 0xFFFFFFFF, 0, _p(offsets), _p(ids) if ids is not None else None, cap, int(counting), C.byref(st)),
                      "rt_%s_list" % name)
        if capacity is None:
            call(None, 0)
            capacity = int(offsets[n])
        capacity = int(capacity)
        ids = np.zeros((capacity, 2), np.int32) if capacity else None
        call(ids, capacity)
        return offsets, ids, st

    def overlap_boxes_list(self, boxes8, capacity=None, cull_mask=0xFF, counting=False):
        """rt_overlap_boxes_list: the blocking host form -> (offsets uint64 (n + 1,), ids int32 (capacity, 2) or None, RtStats; with
        counting its node_visits / tri_tests are those of both walks).  Rows that do not fit `capacity` stay zero."""
        return self._overlap_list_host(np.ascontiguousarray(boxes8, np.float32).reshape(-1, 8), "overlap_boxes", capacity, cull_mask, counting)

    def overlap_triangles_list(self, tris12, capacity=None, cull_mask=0xFF, counting=False):
        """rt_overlap_triangles_list: the blocking host form, as overlap_boxes_list"""
        return self._overlap_list_host(np.ascontiguousarray(tris12, np.float32).reshape(-1, 12), "overlap_triangles", capacity, cull_mask, counting)

    def overlap_scene_triangles_list(self, refs, capacity=None, cull_mask=0xFF, counting=False):
        """rt_overlap_scene_triangles_list: the blocking host form (refs as for overlap_scene_triangles), as overlap_boxes_list"""
        return self._overlap_list_host(_host_refs(refs), "overlap_scene_triangles", capacity, cull_mask, counting)

    def closest_scene_triangle_device(self, refs, cull_mask=0xFF, attributes=False, params=False, stream=None, out=None):
        """rt_closest_scene_triangle_device: closest_triangle_device asked about triangles of the scene itself.  `refs` is
        scene_triangles_device's tensor (triangle_refs packs it, r_max the search radius).  The RayQuery names the candidate triangle;
        quv and hit_kind refer to the source triangle's world image.  Every other argument as for closest_triangle_device.  See
        include/rt_api.h."""
        import torch
        self._check_rays(refs, "closest_scene_triangle_device", 4, "reference", True)
        n = refs.shape[0]
        quv = None
        if out is not None and len(out) == 3:
            quv, out = out[2], tuple(out[:2])
            if params and (quv is None or quv.dtype != torch.float32 or tuple(quv.shape) != (n, 2) or not quv.is_contiguous() or quv.device != refs.device):
                raise ValueError("out quv must be a contiguous float32 (n, 2) tensor on the references' device")
        if not params:
            quv = None
        elif quv is None:
            quv = torch.empty((n, 2), dtype=torch.float32, device=refs.device)

        def call(run, hits, attr):
            if quv is not None:
                quv.record_stream(run)
            return self.L.rt_closest_scene_triangle_device(self.h, n, C.c_void_p(refs.data_ptr()), int(cull_mask) & 0xFFFFFFFF, C.c_void_p(hits.data_ptr()),
                                                           C.c_void_p(attr.data_ptr()) if attr is not None else None,
                                                           C.c_void_p(quv.data_ptr()) if quv is not None else None, C.c_void_p(run.cuda_stream))
        hits, attr = self._device_query(refs, attributes, stream, out, (), call, "rt_closest_scene_triangle_device", cols=4, checked=True)
        res = RayQuery(hits, attr, hit_kind=True)
        res.quv = quv
        return res

    def closest_scene_triangle(self, refs, cull_mask=0xFF, params=False, counting=False):
        """rt_closest_scene_triangle: the blocking host form (refs: TRI_REF_DTYPE records or (n, 4) int32 rows) -> (HIT_DTYPE records,
        RtStats; with counting its node_visits / tri_tests are filled), or with params=True (records, (qu, qv) float32 (n, 2), RtStats)"""
        refs = _host_refs(refs)
        out = np.zeros(len(refs), HIT_DTYPE)
        quv = np.zeros((len(refs), 2), np.float32) if params else None
        st = RtStats()
        self._chk(self.L.rt_closest_scene_triangle(self.h, len(refs), _p(refs), int(cull_mask) & 0xFFFFFFFF, _p(out), _p(quv) if quv is not None else None,
                                                   int(counting), C.byref(st)), "rt_closest_scene_triangle")
        return (out, quv, st) if params else (out, st)

    def closest_instances_device(self, irefs, cull_mask=0xFF, attributes=False, params=False, stream=None, out=None):
        """rt_closest_instances_device: the nearest pair of every pair of bodies.  `irefs` is a contiguous int32 torch tensor (n, 4) on
        this context's GPU (inst, against, the bits of r_max, ignored per row; instance_refs packs it): instance `inst` against every
        other instance (against = -1) or against that one, within r_max.  Returns a RayQuery that names the candidate triangle as
        closest_scene_triangle_device does for the winning source triangle; its `src_prim` is an int32 (n,) tensor, that source
        triangle (-1 on a miss); quv (params=True) and hit_kind refer to its world image.  out = (hits, attr, src_prim) or
        (hits, attr, src_prim, quv) reuses buffers.  See include/rt_api.h."""
        import torch
        self._check_rays(irefs, "closest_instances_device", 4, "record", True)
        n = irefs.shape[0]
        src = quv = None
        if out is not None:
            if len(out) not in (3, 4):
                raise ValueError("out is (hits, attr, src_prim) or (hits, attr, src_prim, quv)")
            src, quv, out = out[2], (out[3] if len(out) == 4 else None), tuple(out[:2])
            if src is None or src.dtype != torch.int32 or tuple(src.shape) != (n,) or not src.is_contiguous() or src.device != irefs.device:
                raise ValueError("out src_prim must be a contiguous int32 (n,) tensor on the records' device")
            if params and (quv is None or quv.dtype != torch.float32 or tuple(quv.shape) != (n, 2) or not quv.is_contiguous() or quv.device != irefs.device):
                raise ValueError("out quv must be a contiguous float32 (n, 2) tensor on the records' device")
        else:
            src = torch.empty((n,), dtype=torch.int32, device=irefs.device)
        if not params:
            quv = None
        elif quv is None:
            quv = torch.empty((n, 2), dtype=torch.float32, device=irefs.device)

        def call(run, hits, attr):
            src.record_stream(run)
            if quv is not None:
                quv.record_stream(run)
            return self.L.rt_closest_instances_device(self.h, n, C.c_void_p(irefs.data_ptr()), int(cull_mask) & 0xFFFFFFFF, C.c_void_p(hits.data_ptr()),
                                                      C.c_void_p(src.data_ptr()), C.c_void_p(attr.data_ptr()) if attr is not None else None,
                                                      C.c_void_p(quv.data_ptr()) if quv is not None else None, C.c_void_p(run.cuda_stream))
        hits, attr = self._device_query(irefs, attributes, stream, out, (), call, "rt_closest_instances_device", cols=4, checked=True)
        res = RayQuery(hits, attr, hit_kind=True)
        res.src_prim = src
        res.quv = quv
        return res

    def closest_instances(self, irefs, cull_mask=0xFF, params=False, counting=False):
        """rt_closest_instances: the blocking host form (irefs: INST_REF_DTYPE records or (n, 4) int32 rows) -> (HIT_DTYPE records,
        src_prim int32 (n,), RtStats; with counting its node_visits / tri_tests are filled: a measurement, they depend on timing), or
        with params=True (records, src_prim, (qu, qv) float32 (n, 2), RtStats)"""
        irefs = _host_irefs(irefs)
        n = len(irefs)
        out = np.zeros(n, HIT_DTYPE)
        src = np.zeros(n, np.int32)
        quv = np.zeros((n, 2), np.float32) if params else None
        st = RtStats()
        self._chk(self.L.rt_closest_instances(self.h, n, _p(irefs), int(cull_mask) & 0xFFFFFFFF, _p(out), _p(src), _p(quv) if quv is not None else None,
                                              int(counting), C.byref(st)), "rt_closest_instances")
        return (out, src, quv, st) if params else (out, src, st)

    def overlap_instances_device(self, irefs, cull_mask=0xFF, any=False, first=False, stream=None, out=None):
        """rt_overlap_instances_device: the intersecting triangle pairs of every pair of bodies.  `irefs` as for
        closest_instances_device (r_max is ignored).  Returns (count, first4): count an int64 (n,) tensor, the number of pairs (with
        any=True 0 or 1, and every record stops at its first contact); first4, with first=True (not with any), an int32 (n, 4)
        tensor (p, inst, prim, 0): the smallest source primitive with a contact and the smallest triangle it touches, -1s when there
        is none; else None.  out = (count, first4) reuses such buffers.  See include/rt_api.h."""
        import torch
        self._check_rays(irefs, "overlap_instances_device", 4, "record", True)
        if any and first:
            raise ValueError("any=True stops at any contact: first must be False")
        n = irefs.shape[0]
        cur = torch.cuda.current_stream(irefs.device)
        if stream is None:
            stream = cur
        if out is None:
            count = torch.empty((n,), dtype=torch.int64, device=irefs.device)
            first4 = torch.empty((n, 4), dtype=torch.int32, device=irefs.device) if first else None
            if stream != cur:   # (allocated for the current stream, written on `stream`)
                count.record_stream(stream)
                if first4 is not None:
                    first4.record_stream(stream)
        else:
            count, first4 = out
            if count is None or count.dtype != torch.int64 or tuple(count.shape) != (n,) or not count.is_contiguous() or count.device != irefs.device:
                raise ValueError("out count must be a contiguous int64 (n,) tensor on the records' device")
            if first and (first4 is None or first4.dtype != torch.int32 or tuple(first4.shape) != (n, 4) or not first4.is_contiguous() or first4.device != irefs.device):
                raise ValueError("out first4 must be a contiguous int32 (n, 4) tensor on the records' device")
            first4 = first4 if first else None

        def call(run):
            return self.L.rt_overlap_instances_device(self.h, n, C.c_void_p(irefs.data_ptr()), int(cull_mask) & 0xFFFFFFFF, OVERLAP_ANY if any else 0,
                                                      C.c_void_p(count.data_ptr()), C.c_void_p(first4.data_ptr()) if first4 is not None else None,
                                                      C.c_void_p(run.cuda_stream))
        if n:
            self._on_stream(stream, (irefs, count, first4), call, "rt_overlap_instances_device")
        return count, first4

    def overlap_instances(self, irefs, cull_mask=0xFF, any=False, first=False, counting=False):
        """rt_overlap_instances: the blocking host form (irefs as for closest_instances) -> (counts uint64 (n,), first4 int32 (n, 4) or
        None, RtStats; with counting its node_visits / tri_tests are filled: a measurement, they depend on timing)"""
        irefs = _host_irefs(irefs)
        n = len(irefs)
        cnt = np.zeros(n, np.uint64)
        first4 = np.zeros((n, 4), np.int32) if first else None
        st = RtStats()
        self._chk(self.L.rt_overlap_instances(self.h, n, _p(irefs), int(cull_mask) & 0xFFFFFFFF, OVERLAP_ANY if any else 0, _p(cnt),
                                              _p(first4) if first4 is not None else None, int(counting), C.byref(st)), "rt_overlap_instances")
        return cnt, first4, st

    def instance_pairs_device(self, irefs, capacity=None, cull_mask=0xFF, above=False, stream=None, out=None):
        """rt_instance_pairs_device: the broad phase over the scene's instances.  `irefs` as for closest_instances_device, r_max the
        margin: row i lists every instance whose canonical box comes within r_max of the box of instance `inst` (against = -1: of
        the others; against >= 0: that one or nothing; above=True: only instances above inst, every unordered pair once).  Returns
        an InstancePairs that unpacks as (offsets, pairs, total): offsets int64 (n + 1,), always complete; pairs int32
        (capacity, 4), row i the records (inst, j, the bits of r_max, 0) in ascending j at pairs[offsets[i]:offsets[i + 1]], written
        if and only if offsets[i + 1] <= capacity (capacity 0: None); total a 0-d view of offsets[n] (reading it is the caller's
        synchronisation).  pairs[:total] is the `irefs` of closest_instances_device and overlap_instances_device as it is.
        capacity=None and out=(offsets, pairs) behave as for overlap_boxes_device_list: a loop keeps one pair buffer and passes it
        through out.  See include/rt_api.h."""
        res = self._overlap_list_device(irefs, "instance_pairs", 4, "record", capacity, cull_mask, stream, out, int32=True, width=4,
                                        flags=INSTANCE_PAIRS_ABOVE if above else 0, suffix="_device")
        return InstancePairs(res.offsets, res.ids)

    def instance_pairs(self, irefs, capacity=None, cull_mask=0xFF, above=False, counting=False):
        """rt_instance_pairs: the blocking host form (irefs as for closest_instances) -> (offsets uint64 (n + 1,), pairs int32
        (capacity, 4) or None, RtStats; with counting its node_visits are TLAS node visits and its tri_tests exact box tests, of
        both walks).  capacity=None: an offsets-only call first, then one with exactly the total.  Rows that do not fit stay zero."""
        irefs = _host_irefs(irefs)
        n = len(irefs)
        offsets = np.zeros(n + 1, np.uint64)
        st = RtStats()

        def call(pairs, cap):
            self._chk(self.L.rt_instance_pairs(self.h, n, _p(irefs), int(cull_mask) & 0xFFFFFFFF, INSTANCE_PAIRS_ABOVE if above else 0, _p(offsets),
                                               _p(pairs) if pairs is not None else None, cap, int(counting), C.byref(st)), "rt_instance_pairs")
        if capacity is None:
            call(None, 0)
            capacity = int(offsets[n])
        capacity = int(capacity)
        pairs = np.zeros((capacity, 4), np.int32) if capacity else None
        call(pairs, capacity)
        return offsets, pairs, st

    def intersect_device_hits(self, rays, max_hits, ray_flags=0, cull_mask=0xFF, words=None, attributes=False, counts=True, stream=None, out=None):
        """rt_intersect_device_hits: every candidate along each ray, the first max_hits of them in (t, inst, prim) order, and their number.
        rays and words as for intersect_device_flags; max_hits 1..16, or 0 for counts only.  Read and written in the order of `stream`
        (default: the current torch stream of the rays' device), with no host synchronisation.  Returns a RayHits of views over one int32
        (n, max_hits, 5) hits buffer, with attributes=True one int32 (n, max_hits, 8) attribute buffer, with counts=True (required when
        max_hits is 0) one int32 (n,) count buffer.  counts=False lets the walk prune beyond the max_hits-th entry.  out = (hits, attr,
        count) reuses such buffers (None where not asked for).  See include/rt_api.h."""
        import torch
        self._check_rays(rays, "intersect_device_hits")
        k = int(max_hits)
        if not 0 <= k <= 16:
            raise ValueError("max_hits must be 0..16, got %d" % k)
        if k == 0 and (attributes or not counts):
            raise ValueError("max_hits 0 counts only: counts=True and attributes=False")
        n = rays.shape[0]
        if words is not None:
            if not isinstance(words, torch.Tensor):
                raise TypeError("words must be a torch tensor, got %s" % type(words).__name__)
            if words.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
                raise ValueError("words must be int32 or uint32, not %s" % words.dtype)
            if words.device != rays.device or not words.is_contiguous() or tuple(words.shape) != (n,):
                raise ValueError("words must be a contiguous (n,) tensor on the rays' device")
        stream, hits, attr, count = self._row_buffers(rays, k, attributes, counts, stream, out)

        def call(run):
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
            return self.L.rt_intersect_device_hits(self.h, n, ptr(rays), ptr(words) if n else None, int(ray_flags) & 0xFFFFFFFF, int(cull_mask) & 0xFFFFFFFF,
                                                   k, ptr(hits), ptr(attr), ptr(count), C.c_void_p(run.cuda_stream))
        if n:
            self._on_stream(stream, (rays, words, hits, attr, count), call, "rt_intersect_device_hits")
        return RayHits(hits, attr, count, n, k)

    def closest_point_device_hits(self, points, max_hits, cull_mask=0xFF, attributes=False, counts=True, stream=None, out=None):
        """rt_closest_point_device_hits: the max_hits nearest triangles of every query point in (d2, inst, prim) order, and the number of
        triangles within the point's radius.  points as for closest_point_device ((n, 4): x, y, z, r_max); max_hits 1..16, or 0 for
        counts only (the sphere-overlap count).  Read and written in the order of `stream`, with no host synchronisation.  Returns a
        RayHits of views over one int32 (n, max_hits, 5) hits buffer (t the distance; entry 0 is closest_point_device's record; entries
        past a point's candidates have prim = inst = -1 and t = r_max), with attributes=True one int32 (n, max_hits, 8) attribute buffer
        (hit_kind: the side of the triangle's plane the point lies on), with counts=True (required when max_hits is 0) one int32 (n,)
        count buffer.  counts=False lets the walk prune beyond the max_hits-th entry.  out = (hits, attr, count) reuses such buffers
        (None where not asked for).  See include/rt_api.h."""
        self._check_rays(points, "closest_point_device_hits", 4, "point")
        k = int(max_hits)
        if not 0 <= k <= 16:
            raise ValueError("max_hits must be 0..16, got %d" % k)
        if k == 0 and (attributes or not counts):
            raise ValueError("max_hits 0 counts only: counts=True and attributes=False")
        n = points.shape[0]
        stream, hits, attr, count = self._row_buffers(points, k, attributes, counts, stream, out)

        def call(run):
            ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
            return self.L.rt_closest_point_device_hits(self.h, n, ptr(points), int(cull_mask) & 0xFFFFFFFF, k, ptr(hits), ptr(attr), ptr(count),
                                                       C.c_void_p(run.cuda_stream))
        if n:
            self._on_stream(stream, (points, hits, attr, count), call, "rt_closest_point_device_hits")
        return RayHits(hits, attr, count, n, k)

    def closest_point_hits(self, points4, max_hits, cull_mask=0xFF, counts=True, counting=False):
        """rt_closest_point_hits: the blocking host form -> (HIT_DTYPE records (n, max_hits) or None, counts uint32 (n,) or None, RtStats;
        with counting its node_visits / tri_tests are filled)"""
        points4 = np.ascontiguousarray(points4, np.float32).reshape(-1, 4)
        n, k = len(points4), int(max_hits)
        hits = np.zeros((n, k), HIT_DTYPE) if k else None
        cnt = np.zeros(n, np.uint32) if counts else None
        st = RtStats()
        self._chk(self.L.rt_closest_point_hits(self.h, n, _p(points4), int(cull_mask) & 0xFFFFFFFF, k & 0xFFFFFFFF, _p(hits) if hits is not None else None,
                                               _p(cnt) if cnt is not None else None, int(counting), C.byref(st)), "rt_closest_point_hits")
        return hits, cnt, st

    def _row_buffers(self, rays, k, attributes, counts, stream, out):
        """the outputs of a list query over the n records of `rays`: int32 (n, k, 5) hits (k > 0), (n, k, 8) attributes and (n,) counts
        where asked for, new or checked from out = (hits, attr, count) -> (the stream to run on, hits, attr, count)"""
        import torch
        n = rays.shape[0]
        cur = torch.cuda.current_stream(rays.device)
        if stream is None:
            stream = cur
        shapes = ((n, k, 5) if k else None, (n, k, 8) if attributes else None, (n,) if counts else None)
        if out is None:
            bufs = [torch.empty(sh, dtype=torch.int32, device=rays.device) if sh is not None else None for sh in shapes]
            if stream != cur:   # (allocated for the current stream, written on `stream`)
                for t in bufs:
                    if t is not None:
                        t.record_stream(stream)
        else:
            bufs = list(out)
            for i, (t, sh, what) in enumerate(zip(bufs, shapes, ("hits", "attributes", "counts"))):
                if sh is None:
                    bufs[i] = None
                elif t is None or t.dtype != torch.int32 or tuple(t.shape) != sh or not t.is_contiguous() or t.device != rays.device:
                    raise ValueError("out %s must be a contiguous int32 %s tensor on the rays' device" % (what, sh))
        return (stream, *bufs)

    def shade_rays_device(self, rays, samples=1, per_sample=True, points=True, stream=None, out=None):
        """rt_shade_rays_device: the frame's shading of caller-generated primary rays.  `rays` is a contiguous float32 torch tensor
        (n_points * samples, 8) on this context's GPU (o.xyz, reserved, d.xyz, tmax per row; d normalised), sample-major: row
        i * n_points + p is sample i of point p.  Read and written in the order of `stream` (default: the current torch stream of that
        device); the call never waits on the host.  Returns (samples_rgba, points_rgba): float32 (n, 4) per-sample colours (alpha 1; 0 for
        a record that is not a ray) and float32 (n_points, 4) per-point averages, each None when not asked for (per_sample / points).
        out = (samples_rgba, points_rgba) reuses such buffers (None where not asked for).  See include/rt_api.h."""
        import torch
        self._check_rays(rays, "shade_rays_device")
        samples = int(samples)
        if samples < 1:
            raise ValueError("samples must be >= 1, got %d" % samples)
        if not (per_sample or points):
            raise ValueError("shade_rays_device needs per_sample or points")
        n = rays.shape[0]
        if n % samples:
            raise ValueError("the ray tensor holds n_points * samples rows: %d rows are not a multiple of %d samples" % (n, samples))
        n_points = n // samples
        cur = torch.cuda.current_stream(rays.device)
        if stream is None:
            stream = cur
        if out is None:
            srgba = torch.empty((n, 4), dtype=torch.float32, device=rays.device) if per_sample else None
            prgba = torch.empty((n_points, 4), dtype=torch.float32, device=rays.device) if points else None
            if stream != cur:   # (allocated for the current stream, written on `stream`)
                for t in (srgba, prgba):
                    if t is not None:
                        t.record_stream(stream)
        else:
            srgba, prgba = out
            for t, want, rows, what in ((srgba, per_sample, n, "samples"), (prgba, points, n_points, "points")):
                if want and (t is None or t.dtype != torch.float32 or tuple(t.shape) != (rows, 4) or not t.is_contiguous() or t.device != rays.device):
                    raise ValueError("out %s must be a contiguous float32 (%d, 4) tensor on the rays' device" % (what, rows))
            srgba = srgba if per_sample else None
            prgba = prgba if points else None

        def call(run):
            return self.L.rt_shade_rays_device(self.h, n_points, samples, C.c_void_p(rays.data_ptr()),
                                               C.c_void_p(srgba.data_ptr()) if srgba is not None else None,
                                               C.c_void_p(prgba.data_ptr()) if prgba is not None else None, C.c_void_p(run.cuda_stream))
        if n:
            self._on_stream(stream, (rays, srgba, prgba), call, "rt_shade_rays_device")
        return srgba, prgba

    def _check_rays(self, rays, name, cols=8, noun="ray", int32=False):
        """the checks of a (n, 8) float32 ray tensor (or, with cols=4 and noun="point", a (n, 4) point tensor; with int32, an int32
        tensor: the (n, 4) references of triangle_refs) on this context's GPU"""
        import torch
        if not isinstance(rays, torch.Tensor):
            raise TypeError("%s takes a torch tensor, got %s" % (name, type(rays).__name__))
        if rays.device.type != "cuda" or rays.device.index != self.device:
            raise ValueError("%s tensor must live on cuda:%d (the context's GPU), not %s" % (noun, self.device, rays.device))
        if rays.dtype != (torch.int32 if int32 else torch.float32):
            raise ValueError("%s tensor must be %s, not %s" % (noun, "int32" if int32 else "float32", rays.dtype))
        if not rays.is_contiguous():
            raise ValueError("%s tensor must be contiguous" % noun)
        if rays.dim() != 2 or rays.shape[1] != cols:
            raise ValueError("%s tensor has shape (n, %d), got %s" % (noun, cols, tuple(rays.shape)))

    def _on_stream(self, stream, tensors, call, name):
        """call(run_stream) -> status, on `stream`; torch's default stream is the null stream, which the C ABI reads as "the context's
        stream" (a non-blocking stream the null stream does not order): then the call goes through a side stream that waits for the
        default stream and that the default stream waits for in turn — no host synchronisation"""
        import torch
        run = stream
        if stream.cuda_stream == 0:
            if getattr(self, "_query_stream", None) is None:
                self._query_stream = torch.cuda.Stream(stream.device)
            run = self._query_stream
            run.wait_stream(stream)
            for t in tensors:
                if t is not None:
                    t.record_stream(run)
        self._chk(call(run), name)
        if run is not stream:
            stream.wait_stream(run)

    def _device_query(self, rays, attributes, stream, out, inputs, call, name, cols=8, checked=False):
        """the common part of intersect_device*: checks (unless the caller has run _check_rays itself: checked=True), output buffers, the
        null-stream detour; call(run_stream, hits, attr) -> status"""
        import torch
        if not checked:
            self._check_rays(rays, "closest_point_device" if cols == 4 else "intersect_device", cols, "point" if cols == 4 else "ray")
        n = rays.shape[0]
        cur = torch.cuda.current_stream(rays.device)
        if stream is None:
            stream = cur
        if out is None:
            hits = torch.empty((n, 5), dtype=torch.int32, device=rays.device)
            attr = torch.empty((n, 8), dtype=torch.int32, device=rays.device) if attributes else None
            if stream != cur:   # (allocated for the current stream, written on `stream`)
                hits.record_stream(stream)
                if attr is not None:
                    attr.record_stream(stream)
        else:
            hits, attr = out
            if hits.dtype != torch.int32 or tuple(hits.shape) != (n, 5) or not hits.is_contiguous() or hits.device != rays.device:
                raise ValueError("out hits must be a contiguous int32 (n, 5) tensor on the rays' device")
            if attributes and (attr is None or attr.dtype != torch.int32 or tuple(attr.shape) != (n, 8) or not attr.is_contiguous() or attr.device != rays.device):
                raise ValueError("out attributes must be a contiguous int32 (n, 8) tensor on the rays' device")
            attr = attr if attributes else None
        if n:
            self._on_stream(stream, (rays, hits, attr) + tuple(inputs), lambda run: call(run, hits, attr), name)
        return hits, attr


class RayQuery:
    """Results of RtContext.intersect_device: views over the hits buffer (int32 (n, 5), rt_hit) and the optional attribute buffer
    (int32 (n, 8), rt_hit_attr).  Misses have prim = inst = -1, and zero position / normal with object_index -1."""

    def __init__(self, hits, attr, hit_kind=False):
        import torch
        self.hits, self.attr = hits, attr
        f = hits[:, 0:3].view(torch.float32)
        self.t, self.u, self.v = f[:, 0], f[:, 1], f[:, 2]
        self.prim, self.inst = hits[:, 3], hits[:, 4]
        if attr is not None:
            self.position = attr[:, 0:3].view(torch.float32)
            self.object_index = attr[:, 3]
            self.normal = attr[:, 4:7].view(torch.float32)
        else:
            self.position = self.normal = self.object_index = None
        # intersect_device_flags with attributes: the hit kind (HIT_KIND_FRONT_FACING / HIT_KIND_BACK_FACING, 0 on a miss); None otherwise
        self.hit_kind = attr[:, 7] if (hit_kind and attr is not None) else None

    def numpy(self):
        """the hit records as rt_intersect returns them (HIT_DTYPE), and the attributes as (n, 8) int32 (or None); synchronises"""
        h = self.hits.cpu().numpy().view(HIT_DTYPE).reshape(-1)
        return h, (self.attr.cpu().numpy() if self.attr is not None else None)


class RayHits:
    """Results of RtContext.intersect_device_hits: views over the hits buffer (int32 (n, K, 5), rt_hit rows), the optional attribute
    buffer (int32 (n, K, 8), rt_hit_attr) and the optional counts (int32 (n,)).  t, u, v, prim, inst are (n, K); position and normal
    (n, K, 3); object_index and hit_kind (n, K).  Entries past a ray's candidates have prim = inst = -1 and t = the ray's tmax, zero
    position / normal, object_index -1 and kind 0.  Views that were not asked for are None."""

    def __init__(self, hits, attr, count, n, k):
        import torch
        self.hits, self.attr, self.count = hits, attr, count
        self.max_hits = k
        if hits is not None:
            f = hits[..., 0:3].view(torch.float32)
            self.t, self.u, self.v = f[..., 0], f[..., 1], f[..., 2]
            self.prim, self.inst = hits[..., 3], hits[..., 4]
        else:
            self.t = self.u = self.v = self.prim = self.inst = None
        if attr is not None:
            self.position = attr[..., 0:3].view(torch.float32)
            self.object_index = attr[..., 3]
            self.normal = attr[..., 4:7].view(torch.float32)
            self.hit_kind = attr[..., 7]
        else:
            self.position = self.normal = self.object_index = self.hit_kind = None

    def numpy(self):
        """(hit records as HIT_DTYPE (n, K), attributes as (n, K, 8) int32, counts as (n,) uint32), None where not asked for; synchronises"""
        h = self.hits.cpu().numpy().view(HIT_DTYPE).reshape(self.hits.shape[0], self.max_hits) if self.hits is not None else None
        a = self.attr.cpu().numpy() if self.attr is not None else None
        c = self.count.cpu().numpy().view(np.uint32) if self.count is not None else None
        return h, a, c


class PointsInside:
    """Results of RtContext.point_inside_device: word, int32 (n,), the vote word of every point (bit 0: inside; bits 8-15: the odd votes
    among the directions taken; bits 16-23: the directions taken), and count, int32 (n, n_dirs), the crossings of every direction, or
    None when not asked for.  inside is bit 0 of word as a bool tensor (computed on the current torch stream when read)."""

    def __init__(self, word, count):
        self.word, self.count = word, count

    @property
    def inside(self):
        return (self.word & 1) != 0

    def numpy(self):
        """(words as (n,) uint32, counts as (n, n_dirs) uint32 or None); synchronises"""
        return (self.word.cpu().numpy().view(np.uint32), self.count.cpu().numpy().view(np.uint32) if self.count is not None else None)


class BoxOverlaps:
    """Results of RtContext.overlap_boxes_device: ids, int32 (n, max_ids, 2) rows of (inst, prim) in ascending order with (-1, -1) past a
    box's candidates, and count, int32 (n,), the number of candidates (not capped at max_ids).  inst and prim are (n, max_ids) views.
    What was not asked for is None."""

    def __init__(self, ids, count):
        self.ids, self.count = ids, count
        self.inst = ids[..., 0] if ids is not None else None
        self.prim = ids[..., 1] if ids is not None else None

    def numpy(self):
        """(counts as (n,) uint32, ids as (n, max_ids, 2) int32), None where not asked for; synchronises"""
        return (self.count.cpu().numpy().view(np.uint32) if self.count is not None else None,
                self.ids.cpu().numpy() if self.ids is not None else None)


class OverlapList:
    """Results of RtContext.overlap_*_device_list: offsets, int64 (n + 1,), and ids, int32 (capacity, 2) rows of (inst, prim) or None;
    row i is ids[offsets[i]:offsets[i + 1]] if offsets[i + 1] <= capacity.  total is a 0-d view of offsets[n]: reading it (int(),
    .item()) synchronises."""

    def __init__(self, offsets, ids):
        self.offsets, self.ids = offsets, ids
        self.total = offsets[-1]

    def numpy(self):
        """(offsets as (n + 1,) uint64, ids as (capacity, 2) int32 or None); synchronises"""
        return self.offsets.cpu().numpy().view(np.uint64), self.ids.cpu().numpy() if self.ids is not None else None


class InstancePairs:
    """Results of RtContext.instance_pairs_device: offsets, int64 (n + 1,); pairs, int32 (capacity, 4) rows of (inst, against, the bits
    of r_max, 0) or None; total, a 0-d view of offsets[n] (reading it synchronises).  Unpacks as (offsets, pairs, total)."""

    def __init__(self, offsets, pairs):
        self.offsets, self.pairs = offsets, pairs
        self.total = offsets[-1]

    def __iter__(self):
        return iter((self.offsets, self.pairs, self.total))

    def numpy(self):
        """(offsets as (n + 1,) uint64, pairs as (capacity, 4) int32 or None); synchronises"""
        return self.offsets.cpu().numpy().view(np.uint64), self.pairs.cpu().numpy() if self.pairs is not None else None


def triangle_records(vertices, faces, r_max=0.0):
    """the (nf, 12) float32 records of overlap_triangles_device / overlap_triangles and closest_triangle_device / closest_triangle
    (P0.xyz, r_max, P1.xyz, 0, P2.xyz, 0 per row) of the triangles `faces` (nf, 3) indexes in `vertices` (nv, 3).  `r_max` (a scalar or
    (nf,)) is the search radius of the closest-triangle query; the overlap query ignores it.  torch tensors stay on their device (torch
    indexing, no host copy); anything else goes through numpy."""
    try:
        import torch
        is_t = isinstance(vertices, torch.Tensor)
    except ImportError:
        is_t = False
    if is_t:
        f = torch.as_tensor(faces, device=vertices.device).reshape(-1, 3).long()
        rec = torch.zeros((f.shape[0], 3, 4), dtype=torch.float32, device=vertices.device)
        rec[:, :, :3] = vertices.reshape(-1, 3).to(torch.float32)[f]
        rec[:, 0, 3] = torch.as_tensor(r_max, device=vertices.device).to(torch.float32)
        return rec.reshape(-1, 12)
    f = np.asarray(faces.cpu() if hasattr(faces, "cpu") else faces).reshape(-1, 3).astype(np.int64)
    rec = np.zeros((len(f), 3, 4), np.float32)
    rec[:, :, :3] = np.asarray(vertices, np.float32).reshape(-1, 3)[f]
    rec[:, 0, 3] = np.asarray(r_max.cpu() if hasattr(r_max, "cpu") else r_max, np.float32)
    return rec.reshape(-1, 12)


def _host_refs(refs):
    """host references as contiguous (n, 4) int32 rows: TRI_REF_DTYPE records or anything triangle_refs returns for numpy input"""
    refs = np.asarray(refs)
    if refs.dtype == TRI_REF_DTYPE:
        return np.ascontiguousarray(refs).view(np.int32).reshape(-1, 4)
    if refs.dtype != np.int32:
        raise ValueError("references must be TRI_REF_DTYPE records or int32 rows, not %s" % refs.dtype)
    return np.ascontiguousarray(refs).reshape(-1, 4)


def _host_irefs(irefs):
    """host instance-pair records as contiguous (n, 4) int32 rows: INST_REF_DTYPE records or anything instance_refs returns for numpy input"""
    irefs = np.asarray(irefs)
    if irefs.dtype == INST_REF_DTYPE:
        return np.ascontiguousarray(irefs).view(np.int32).reshape(-1, 4)
    if irefs.dtype != np.int32:
        raise ValueError("records must be INST_REF_DTYPE records or int32 rows, not %s" % irefs.dtype)
    return np.ascontiguousarray(irefs).reshape(-1, 4)


def instance_refs(inst, against=REF_AGAINST_OTHERS, r_max=float("inf")):
    """the (n, 4) int32 rows (rt_inst_ref: inst, against, the bits of r_max, 0) of closest_instances* and overlap_instances*: instance
    `inst` as the query, against every other instance (against = -1) or against that instance only.  inst, against and r_max broadcast
    against each other ((n,) or scalars).  torch tensors stay on their device; anything else goes through numpy (the rows then view as
    INST_REF_DTYPE)."""
    try:
        import torch
        dev = next((x.device for x in (inst, against, r_max) if isinstance(x, torch.Tensor)), None)
    except ImportError:
        dev = None
    if dev is not None:
        i, a, r = torch.broadcast_tensors(*(torch.as_tensor(x, device=dev).reshape(-1) for x in (inst, against, r_max)))
        rec = torch.zeros((i.shape[0], 4), dtype=torch.int32, device=dev)
        rec[:, 0] = i.to(torch.int32); rec[:, 1] = a.to(torch.int32)
        rec[:, 2] = r.to(torch.float32).contiguous().view(torch.int32)
        return rec
    i, a, r = np.broadcast_arrays(*(np.asarray(x).reshape(-1) for x in (inst, against, r_max)))
    rec = np.zeros((len(i), 4), np.int32)
    rec[:, 0] = i.astype(np.int64).astype(np.int32); rec[:, 1] = a.astype(np.int64).astype(np.int32)
    rec[:, 2] = np.ascontiguousarray(r, np.float32).view(np.int32)
    return rec


def triangle_refs(inst, prim, against=REF_AGAINST_OTHERS, r_max=float("inf")):
    """the (n, 4) int32 rows (rt_tri_ref: inst, prim, against, the bits of r_max) of scene_triangles_device, overlap_scene_triangles* and
    closest_scene_triangle*: triangle `prim` of instance `inst` as the query, against every other instance (against = -1) or against
    that instance only.  inst, prim, against and r_max broadcast against each other ((n,) or scalars).  torch tensors stay on their
    device; anything else goes through numpy (the rows then view as TRI_REF_DTYPE)."""
    try:
        import torch
        dev = next((x.device for x in (inst, prim, against, r_max) if isinstance(x, torch.Tensor)), None)
    except ImportError:
        dev = None
    if dev is not None:
        i, p, a, r = torch.broadcast_tensors(*(torch.as_tensor(x, device=dev).reshape(-1) for x in (inst, prim, against, r_max)))
        rec = torch.empty((i.shape[0], 4), dtype=torch.int32, device=dev)
        rec[:, 0] = i.to(torch.int32); rec[:, 1] = p.to(torch.int32); rec[:, 2] = a.to(torch.int32)
        rec[:, 3] = r.to(torch.float32).contiguous().view(torch.int32)
        return rec
    i, p, a, r = np.broadcast_arrays(*(np.asarray(x).reshape(-1) for x in (inst, prim, against, r_max)))
    rec = np.empty((len(i), 4), np.int32)
    rec[:, 0] = i.astype(np.int64).astype(np.int32); rec[:, 1] = p.astype(np.int64).astype(np.int32); rec[:, 2] = a.astype(np.int64).astype(np.int32)
    rec[:, 3] = np.ascontiguousarray(r, np.float32).view(np.int32)
    return rec


def capsule_records(p0, p1, r_max):
    """the (n, 8) float32 records of closest_segment_device / closest_segment (P0.xyz, r_max, P1.xyz, 0 per row) of the segments from
    `p0` (n, 3) to `p1` (n, 3) with the search radii `r_max` ((n,) or a scalar; for a capsule, at least its radius).  torch tensors stay
    on their device; anything else goes through numpy."""
    try:
        import torch
        is_t = isinstance(p0, torch.Tensor)
    except ImportError:
        is_t = False
    if is_t:
        a = p0.reshape(-1, 3).to(torch.float32)
        rec = torch.zeros((a.shape[0], 8), dtype=torch.float32, device=a.device)
        rec[:, 0:3] = a
        rec[:, 4:7] = torch.as_tensor(p1, device=a.device).reshape(-1, 3).to(torch.float32)
        rec[:, 3] = torch.as_tensor(r_max, device=a.device).to(torch.float32)
        return rec
    a = np.asarray(p0, np.float32).reshape(-1, 3)
    rec = np.zeros((len(a), 8), np.float32)
    rec[:, 0:3] = a
    rec[:, 4:7] = np.asarray(p1, np.float32).reshape(-1, 3)
    rec[:, 3] = np.asarray(r_max, np.float32)
    return rec


def check_builders(verts6, idx):
    """rt_debug_check_builders: host-only invariants of the BVH builders; returns (status, stats dict)."""
    verts6 = np.ascontiguousarray(verts6, np.float32)
    idx = np.ascontiguousarray(idx, np.uint32)
    out = np.zeros(8, np.uint64)
    rc = lib().rt_debug_check_builders(_p(verts6), verts6.size, _p(idx), idx.size, _p(out))
    keys = ("nodes", "leaves", "depth", "max_leaf", "bvh4_nodes", "bvh4_stack_need", "violations", "reached")
    return rc, dict(zip(keys, (int(x) for x in out)))


def host_blas(verts6, idx):
    """rt_debug_host_blas: the quantized BVH2 (links local to the mesh) and the triangle packets of the host builder, without a GPU;
    returns (status, dict of nodes, packets, q_lo, q_scale)."""
    verts6 = np.ascontiguousarray(verts6, np.float32)
    idx = np.ascontiguousarray(idx, np.uint32)
    n = idx.size // 3
    nodes, packets, out = np.zeros(max(1, n), NODEQ_DTYPE), np.zeros(max(1, n), TRI_PACKET_DTYPE), np.zeros(8, np.uint64)
    rc = lib().rt_debug_host_blas(_p(verts6), verts6.size, _p(idx), idx.size, _p(nodes), nodes.nbytes, _p(packets), packets.nbytes, _p(out))
    bits = out[2:8].astype(np.uint32).view(np.float32)
    return rc, {"nodes": nodes[:int(out[0])].copy(), "packets": packets[:int(out[1])].copy(), "q_lo": bits[:3].copy(), "q_scale": bits[3:].copy()}
