"""Every consumer of a built scene, run once over one set of query records, and the assertions on their buffers that do not depend on
the scene: shared by tests/test_instance_records.py (bad instance records) and tests/test_bad_vertices.py (bad vertex positions).
consume(c, rays, records, any_tmax, W, H) -> {buffer name: numpy array}: closest and any hits, flags with attributes, the 4 nearest
hits with counts, point-inside votes and counts, shaded rays, closest points, sphere sweeps, box and triangle overlaps, signed
distances, a frame with the default tunables and one without coverage mask and pixel beams."""
import numpy as np

from tests import inside_reference as ir
from vulkan_raytracing_amd import api

RAY_CONSUMERS = ("closest", "closest_attr", "any", "flags", "flags_attr", "hits4", "hits4_count", "inside", "inside_count", "shade_s", "shade_p",
                 "frame", "frame_counts", "frame_plain", "frame_plain_counts")
WORLD_CONSUMERS = ("cp", "cp_attr", "sweep", "sweep_attr", "boxes_ids", "boxes_count", "tris_ids", "tris_count", "sd", "sd_attr")


def dev(a, dtype=np.float32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda:0")


def consume(c, rays, q, any_tmax, W, H):
    """every consumer once over the scene's query records -> {buffer name: numpy array}"""
    import torch
    rays = dev(rays)
    sh = rays.clone(); sh[:, 7] = any_tmax
    out = {}
    r = c.intersect_device(rays, attributes=True)
    out["closest"], out["closest_attr"] = r.hits, r.attr
    # any hit: whether the segment is blocked — which of several blockers a walk meets first depends on the tree (tests/test_device_tlas.py),
    # and the tree of a scene with a void record is not its twin's
    out["any"] = c.intersect_device(sh, any_hit=True).inst >= 0
    r = c.intersect_device_flags(rays, ray_flags=api.RAY_FLAG_CULL_BACK_FACING, attributes=True)
    out["flags"], out["flags_attr"] = r.hits, r.attr
    r = c.intersect_device_hits(rays, 4, counts=True)
    out["hits4"], out["hits4_count"] = r.hits, r.count
    pts = dev(q["points"])
    r = c.point_inside_device(pts, n_dirs=3, counts=True)
    out["inside"], out["inside_count"] = r.word, r.count
    out["shade_s"], out["shade_p"] = c.shade_rays_device(rays, samples=2)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out.update(consume_world(c, q))
    out.update(frames(c, W, H))
    return out


def consume_world(c, q):
    """the world-space consumers (WORLD_CONSUMERS: closest points, sweeps, box and triangle overlaps, signed distances)"""
    import torch
    out = {}
    pts = dev(q["points"])
    r = c.closest_point_device(pts, attributes=True)
    out["cp"], out["cp_attr"] = r.hits, r.attr
    r = c.sweep_spheres_device(dev(q["sweeps"]), attributes=True)
    out["sweep"], out["sweep_attr"] = r.hits, r.attr
    r = c.overlap_boxes_device(dev(q["boxes"]), max_ids=16)
    out["boxes_ids"], out["boxes_count"] = r.ids, r.count
    r = c.overlap_triangles_device(dev(q["tris"]), max_ids=16)
    out["tris_ids"], out["tris_count"] = r.ids, r.count
    r = c.signed_distance_device(pts, n_dirs=3, attributes=True)
    out["sd"], out["sd_attr"] = r.hits, r.attr
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def frames(c, W, H):
    out = {}
    for key, on in (("frame", 1), ("frame_plain", 0)):
        c.set_param("primary_cover", on); c.set_param("pixel_beams", on)
        try:
            img, st = c.trace(W, H)
        finally:
            c.set_param("primary_cover", 1); c.set_param("pixel_beams", 1)
        out[key] = img
        out[key + "_counts"] = np.array([st.rays_primary, st.rays_secondary, st.rays_shadow], np.int64)
    return out


def assert_same(got, want, keys, what, other="the twin scene's"):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), \
            "%s: buffer %s differs from %s in %d of %d bytes" % (what, k, other, int((got[k].view(np.uint8) != want[k].view(np.uint8)).sum()), got[k].nbytes)


def sign_split(h):
    """(the hit records as words with the sign bit of t cleared, the sign bits): tests/test_point_inside.py"""
    raw = np.ascontiguousarray(h).view(np.uint32).reshape(len(h), 5).copy()
    sign = raw[:, 0] >> 31
    raw[:, 0] &= 0x7FFFFFFF
    return raw, sign


def check_signed_distance(got, what):
    """rt_signed_distance_device is this run's rt_closest_point_device apart from the sign bit of t, which is bit 0 of this run's
    rt_point_inside_device word (tests/test_point_inside.py test_signed_distance): the records, the attributes, the vote.  With the
    words held to the oracle over the twin records, the vote of a signed distance never counts a void or non-invertible record."""
    raw, sign = sign_split(got["sd"])
    craw, csign = sign_split(got["cp"])
    assert np.array_equal(raw, craw) and got["sd_attr"].tobytes() == got["cp_attr"].tobytes(), what
    assert np.array_equal(sign, csign | (got["inside"].view(np.uint32) & 1)), what
    assert np.array_equal(got["inside"].view(np.uint32), ir.words(got["inside_count"].view(np.uint32), 3, True)), what
