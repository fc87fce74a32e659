"""One context family lives through a scripted history; after every step its results are held to the standard of tests/exact.py.

Every other GPU test builds its scene on a fresh context, so the suite shows that each STATE of the library gives the oracle's bits,
not that the way it got there does not matter.  The host side keeps a lot from one call to the next: allocations sized by the largest
call so far, counter blocks and coverage masks one frame clears for the next, hints read from the previous frame, the LRU of jitter
tables, kept light records, the double-buffered instance records.  The scripts of tests/history_steps.py take ONE family (a root, and
frame slots where a track says so) through those histories:

  track A  one context, every kind of change (frame size, spp and depth, shards, 8-bit formats, instance source and count, batches,
           shading tables, sky, light, tunables, counting frames, rejected calls), as a fixed list and two seeded shuffles of it;
  track B  tiny and large frames behind each other, alone and on a family of four (the previous frame's hints size this frame's grids);
  track C  more jitter-table keys than the cache holds, with a frame pending across the evictions;
  track D  every query and shading call at 5000 -> 37 -> 1 -> 5000 records and across geometry, refit and instance changes;
  track E  geometry replaced under a family, destroy orders, the slot limit, and device memory over 30 create / destroy cycles.

A frame must equal the oracle's bit for bit, with the oracle's ray counts; a query or shading result must equal, byte for byte, that of
a fresh context given only that step's state and that one call (and, once per kind, the fresh result is held to the kind's CPU
reference).  A failure names the script, the step's index and its description."""
import os
import time

import numpy as np
import pytest

from oracle import ingest, oracle
from tests import closest_hits_reference as chr_
from tests import closest_reference as cr
from tests import history_steps as hs
from tests import inside_reference as ir
from tests import overlap_reference as orf
from tests import scenes
from tests import segment_reference as sgr
from tests import sweep_reference as sr
from tests import triangle_distance_reference as tdr
from tests import triangle_overlap_reference as tor
from tests.exact import assert_frame_equals_oracle, assert_hits_equal_oracle
from tests.shade_reference import average_points, shade_samples
from vulkan_raytracing_amd import RtContext, api, host, tiling
from vulkan_raytracing_amd.api import HIT_DTYPE, INSTANCE_DTYPE, MATERIAL_DTYPE, MATERIAL_TYPE_OF_INSTANCE, RtError

RES = scenes.RES
TEAPOT, CUBE = os.path.join(RES, "teapot.obj"), os.path.join(RES, "cube.obj")
RT_ERR_INVALID_ARGUMENT, RT_ERR_NOT_READY = 1, 2
ORACLE_THREADS = 16


def counts(st):
    return (int(st.rays_primary), int(st.rays_secondary), int(st.rays_shadow))


class StepFailed(AssertionError):
    pass


def run_script(name, steps, do):
    """do(step) for every step; a failure reads "script <name>, step 7 (small frame after large): ..." """
    for i, step in enumerate(steps):
        try:
            do(step)
        except (AssertionError, RtError, pytest.fail.Exception) as e:
            raise StepFailed("script %s, step %d (%s): %s" % (name, i, step["desc"], e)) from e


def expect_error(call, code, ctx, what):
    with pytest.raises(RtError) as e:
        call()
    assert e.value.code == code, (what, e.value.code, str(e.value))
    assert ctx.L.rt_last_error(ctx.h), what


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- track A's world: the state a script has reached, the oracle that follows it, the context family ------------------------------------

def sky_faces(w, h):
    """scenes.synthetic_skybox for square faces; its pattern on w x h faces otherwise"""
    if w == h:
        return scenes.synthetic_skybox(w, seed=7 + w)
    rng = np.random.default_rng(1000 * w + h)
    yy, xx = np.mgrid[0:h, 0:w]
    faces = []
    for f in range(6):
        img = np.zeros((h, w, 4), np.uint8)
        img[..., 0] = (xx * 255 // (w - 1) + 37 * f) % 256
        img[..., 1] = (yy * 255 // (h - 1) + 91 * f) % 256
        img[..., 2] = rng.integers(0, 256, (h, w))
        img[..., 3] = 255
        faces.append(img)
    return faces


def instance_records(count, t):
    """the reference's two instances at animation time t; for count > 2 a ring of cubes (and a few teapots) about them that turns with t"""
    anim = host.SceneAnimation()
    if t:
        anim.animate(t)
    base = anim.instances((0, 1))
    if count == 2:
        return base
    out = [base[0], base[1]]
    for k in range(count - 2):
        ang = 2.0 * np.pi * k / (count - 2) + t
        m = ingest.mat_translate(ingest.mat_rotate_y(ingest.mat_identity(), np.float32(ang)), (0.0, 0.4 * (k % 5) - 1.0, 6.0 + 0.5 * (k % 3) + t))
        mesh = 0 if k % 13 == 5 else 1
        out.append(host.make_instance(ingest.glm_to_vulkan(m), mesh, mesh))
    return np.asarray(out, INSTANCE_DTYPE)


def device_records(recs):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1, INSTANCE_DTYPE.itemsize).copy()).to("cuda:0")
    torch.cuda.synchronize()
    return t


class World:
    """teapot + cube under a synthetic sky: the state of hs.BASE and what the steps make of it.  ctx None: the oracle alone (CPU)."""

    def __init__(self, ctx=None, with_slot=False):
        self.geom = host.SceneGeometry([TEAPOT, CUBE])
        self.orc = oracle.OracleScene()
        self.orc.set_geometry(self.geom.verts, self.geom.idx, self.geom.ranges)
        self.state = dict(hs.BASE)
        self.refs = {}
        n_prims = len(self.geom.idx) // 3
        a = np.zeros(4, MATERIAL_DTYPE)
        a[0] = ((0.1, 0.2, 0.3), 12.0, (0.9, 0.3, 0.5), 1.3, (0.2, 0.2, 0.2), MATERIAL_TYPE_OF_INSTANCE)
        a[1] = ((0.3, 0.1, 0.1), 50.0, (0.3, 0.8, 0.5), 1.5, (0.6, 0.6, 0.6), 0)
        a[2] = ((0.2, 0.2, 0.2), 10.0, (0.5, 0.5, 0.5), 1.7, (0.2, 0.2, 0.2), 1)
        a[3] = ((0.05, 0.3, 0.2), 3.0, (0.1, 0.9, 0.9), 1.1, (0.9, 0.9, 0.9), 2)
        b = np.zeros(2, MATERIAL_DTYPE)
        b[0] = ((0.2, 0.1, 0.3), 30.0, (0.4, 0.4, 0.9), 1.4, (0.5, 0.5, 0.5), MATERIAL_TYPE_OF_INSTANCE)
        b[1] = ((0.3, 0.3, 0.1), 7.0, (0.9, 0.8, 0.2), 1.2, (0.3, 0.3, 0.3), 0)
        self.tables = {None: (None, None), "A": (a, ((np.arange(n_prims) * 7 // 5) % 4).astype(np.uint32)),
                       "B": (b, ((np.arange(n_prims) // 3) % 2).astype(np.uint32))}
        self.ctx, self.pend = ctx, None
        if ctx is not None:
            ctx.upload_geometry(self.geom.verts, self.geom.idx, self.geom.ranges)
            ctx.set_instances(instance_records(2, 0.0))
            ctx.set_uniforms(self.uniforms())
            ctx.set_skybox(sky_faces(*self.state["sky"]))
            if with_slot:
                self.pend = ctx.frame_slot()

    def close(self):
        if self.pend is not None:
            self.pend.close()
        if self.ctx is not None:
            self.ctx.close()

    def uniforms(self, **over):
        st = dict(self.state, **over)
        u = host.default_uniforms(max_bounce_count=st["depth"], samples_per_pixel=st["spp"], center_object_type=1, orbiting_object_type=0,
                                  orbiting_object_primitive_offset=self.geom.orbiting_primitive_offset,
                                  orbiting_object_vertex_offset=self.geom.orbiting_vertex_offset)
        if st["light"] is not None:
            u[0]["light_position"][:3] = st["light"]
        return u

    def types(self):
        n = self.state["count"]
        return [] if self.state["types"] is None else ([2, 1] + [k % 3 for k in range(n - 2)])

    def set_oracle(self, instances=None, uniforms=None):
        """the oracle in the state the script has reached (or with a batch frame's instances and uniforms)"""
        st = self.state
        inst = instance_records(st["count"], st["time"]) if instances is None else instances
        self.orc.set_instances([inst[i].tobytes() for i in range(len(inst))])
        self.orc.set_uniforms((self.uniforms() if uniforms is None else uniforms).tobytes())
        self.orc.set_skybox(sky_faces(*st["sky"]))
        self.orc.set_materials(*self.tables[st["materials"]])
        self.orc.set_instance_types(self.types())

    def reference(self, W, H, rows=None):
        """(the oracle's frame, its ray counts) in the current state; rows: only these row ranges [(y0, y1)] are rendered and counted"""
        st = self.state
        key = (W, H, tuple(rows) if rows else None) + tuple((k, st[k]) for k in ("spp", "depth", "light", "count", "time", "materials", "types", "sky"))
        self.set_oracle()
        if key not in self.refs:
            if rows is None:
                self.refs[key] = self.orc.render(W, H, threads=ORACLE_THREADS)
            else:
                ref, rc = np.zeros((H, W, 4), np.float32), np.zeros(3, np.uint64)
                for y0, y1 in rows:
                    part, c = self.orc.render(W, H, y0=y0, y1=y1, threads=ORACLE_THREADS)
                    ref[y0:y1] = part[y0:y1]
                    rc += c
                self.refs[key] = (ref, rc)
        return self.refs[key]

    def check(self, img, rays, W, H):
        ref, rc = self.reference(W, H)
        assert_frame_equals_oracle(img, self.orc, W, H, ref=ref, bgra=self.state["bgra"])
        assert tuple(rays) == tuple(int(x) for x in rc), ("ray counts", tuple(rays), tuple(int(x) for x in rc))

    # ---- the ops of a track A step ------------------------------------------------------------------------------------------------
    def do(self, step):
        getattr(self, "op_" + step["op"])(step)

    def size(self, step):
        if step.get("size"):
            self.state["size"] = step["size"]
        return hs.SIZES[self.state["size"]]

    def op_frame(self, step):
        W, H = self.size(step)
        img, st = self.ctx.trace(W, H, counting=step["mode"] == "counting")
        self.check(img, counts(st), W, H)

    def op_uniforms(self, step):
        for k in ("spp", "depth", "light"):
            if k in step:
                self.state[k] = step[k]
        self.ctx.set_uniforms(self.uniforms())

    def op_param(self, step):
        self.ctx.set_param(step["name"], step["value"])
        if step["name"] in ("output_rgba8", "output_bgra8"):
            self.state["rgba8"] = bool(step["value"])
            self.state["bgra"] = bool(step["value"]) and step["name"] == "output_bgra8"

    def op_instances(self, step):
        self.state.update(count=step["count"], source=step["source"], time=step["time"])
        recs = instance_records(step["count"], step["time"])
        if step["source"] == "host":
            self.ctx.set_instances(recs, update=step["update"])
        else:
            self.ctx.set_instances_device(device_records(recs), update=step["update"])
        self.ctx.set_uniforms(self.uniforms())          # (a batch's uniforms were the batch's)

    def batch_frames(self, K):
        us, insts = [], []
        for k in range(K):
            u = self.uniforms()
            u[0]["position"][:3] = (0.4 * k - 0.5, 0.3 * k, 20.0 - 0.7 * k)
            u[0]["light_position"][:3] = (5.0 - k, 5.0 + 0.5 * k, 5.0)
            us.append(u)
            insts.append(instance_records(2, 0.1 * (k + 1)))
        return insts, us

    def render_batch(self, K, W, H):
        import torch
        insts, us = self.batch_frames(K)
        buf = torch.zeros((K, H, W, 4), dtype=torch.float32, device="cuda:0")
        self.ctx.trace_shard_batch(W, H, H, 0, 1, buf.data_ptr(), buf.numel() * 4, stream_ptr())
        got = counts(self.ctx.stats())
        out = buf.cpu().numpy()
        total = np.zeros(3, np.uint64)
        for k in range(K):
            self.set_oracle(insts[k], us[k])
            ref, rc = self.orc.render(W, H, threads=ORACLE_THREADS)
            assert_frame_equals_oracle(out[k], self.orc, W, H, ref=ref)
            total += rc
        assert got == tuple(int(x) for x in total), ("ray counts of the batch", got, total)

    def op_batch(self, step):
        K = step["K"]
        W, H = self.size(step)
        insts, us = self.batch_frames(K)
        self.ctx.set_batch(np.stack(insts), np.concatenate(us), update=step.get("update", False))
        self.render_batch(K, W, H)

    def op_materials(self, step):
        self.state["materials"] = step["which"]
        self.ctx.set_materials(*self.tables[step["which"]])

    def op_types(self, step):
        self.state["types"] = step["which"]
        self.ctx.set_instance_types(self.types())

    def op_sky(self, step):
        self.state["sky"] = (step["w"], step["h"])
        self.ctx.set_skybox(sky_faces(step["w"], step["h"]))

    def op_shards(self, step):
        import torch
        W, H = self.size(step)
        band, n = step["band"], step["n"]
        rows_max = tiling.max_shard_rows(H, band, n)
        side = torch.cuda.Stream()
        shards, total = [], np.zeros(3, np.int64)
        for s in range(n):
            buf = torch.zeros((rows_max, W, 4), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            # (odd shards on a stream of the caller's)
            self.ctx.trace_shard(W, H, band, s, n, buf.data_ptr(), buf.numel() * 4, side.cuda_stream if s % 2 else stream_ptr())
            self.ctx.synchronize()
            total += counts(self.ctx.stats())
            shards.append(buf.cpu().numpy())
        self.check(tiling.assemble(shards, H, W, band), total, W, H)

    def op_empty_shard(self, step):
        import torch
        W, H = self.size(step)
        assert tiling.shard_rows(H, step["band"], step["shard"], step["n"]) == 0
        buf = torch.full((1, W, 4), 7.25, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        self.ctx.trace_shard(W, H, step["band"], step["shard"], step["n"], buf.data_ptr(), buf.numel() * 4, stream_ptr())
        self.ctx.synchronize()
        assert counts(self.ctx.stats()) == (0, 0, 0)
        assert bool((buf == 7.25).all()), "a shard of 0 rows wrote pixels"

    def op_reject(self, step):
        """a call that must fail, directly behind a submitted frame that is collected after it; then the next valid frame"""
        import torch
        kind = step["kind"]
        W, H = self.size(step)
        ctx, pend = self.ctx, self.pend
        u, recs = self.uniforms(), instance_records(2, 0.0)
        assert self.state == dict(hs.BASE, size=self.state["size"]), "rejected calls start from the base state"
        pend.set_instances(recs)
        pend.set_uniforms(u)
        if kind in ("spp0", "depth70"):
            bad = u.copy()
            if kind == "spp0":
                bad[0]["samples_per_pixel"] = 0
            else:
                bad[0]["max_bounce_count"] = 70
            pend.trace_async(W, H)
            ctx.set_uniforms(bad)
            expect_error(lambda: ctx.trace(W, H), RT_ERR_INVALID_ARGUMENT, ctx, kind)
            img, st = pend.trace_wait()
            self.check(img, counts(st), W, H)
            # on ONE context: a frame submitted with trace_shard, the rejected call right behind it on the same stream
            ctx.set_uniforms(u)
            buf = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
            buf2 = torch.full((H, W, 4), 7.25, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            ctx.trace_shard(W, H, H, 0, 1, buf.data_ptr(), buf.numel() * 4, stream_ptr())
            ctx.set_uniforms(bad)
            expect_error(lambda: ctx.trace_shard(W, H, H, 0, 1, buf2.data_ptr(), buf2.numel() * 4, stream_ptr()), RT_ERR_INVALID_ARGUMENT, ctx, kind)
            ctx.synchronize()
            self.check(buf.cpu().numpy(), counts(ctx.stats()), W, H)
            assert bool((buf2 == 7.25).all()), "the rejected call wrote pixels"
            ctx.set_uniforms(u)
        elif kind == "update_count":
            three = instance_records(3, 0.0)
            pend.trace_async(W, H)
            expect_error(lambda: pend.set_instances(three, update=True), RT_ERR_INVALID_ARGUMENT, pend, kind)   # behind its own pending frame
            expect_error(lambda: ctx.set_instances(three, update=True), RT_ERR_INVALID_ARGUMENT, ctx, kind)
            expect_error(lambda: ctx.set_instances_device(device_records(recs), update=True), RT_ERR_INVALID_ARGUMENT, ctx, kind)   # (a host build)
            img, st = pend.trace_wait()
            self.check(img, counts(st), W, H)
        elif kind == "uniforms_in_batch":
            insts, us = self.batch_frames(2)
            ctx.set_batch(np.stack(insts), np.concatenate(us))
            pend.trace_async(W, H)
            other = u.copy()
            other[0]["samples_per_pixel"] = 5
            expect_error(lambda: ctx.set_uniforms(other), RT_ERR_NOT_READY, ctx, kind)
            expect_error(lambda: ctx.trace(W, H), RT_ERR_NOT_READY, ctx, kind)          # (a batch is rendered with trace_shard_batch)
            img, st = pend.trace_wait()
            self.check(img, counts(st), W, H)
            self.render_batch(2, W, H)                                                  # the batch is the one that was set
            ctx.set_instances(recs)
            ctx.set_uniforms(u)
        else:
            raise ValueError(kind)
        img, st = ctx.trace(W, H)                                                       # the very next valid step
        self.check(img, counts(st), W, H)


# ---- CPU: the premises of the scripts ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("script", hs.TRACK_A_SCRIPTS)
def test_track_a_scripts_hold_every_required_transition(script):
    steps = hs.track_a(script)
    tags = {s["tag"] for s in steps if "tag" in s}
    assert tags >= hs.REQUIRED_TAGS, sorted(hs.REQUIRED_TAGS - tags)
    assert len(steps) == sum(len(t[1]) for t in hs.TRANSITIONS) and all(s["desc"] for s in steps)
    if script != "fixed":
        assert [s["desc"] for s in steps] != [s["desc"] for s in hs.track_a("fixed")]
    # every transition ends in the base state, whatever precedes it: followed on the CPU with the interpreter's own bookkeeping
    w = World()
    keep = {"frame": w.size, "batch": w.size, "reject": w.size, "shards": w.size, "empty_shard": w.size}
    for name, tr in hs.TRANSITIONS:
        w.state = dict(hs.BASE)
        for s in tr:
            if s["op"] in keep:
                keep[s["op"]](s)
            elif s["op"] in ("uniforms",):
                w.state.update({k: s[k] for k in ("spp", "depth", "light") if k in s})
            elif s["op"] == "param" and s["name"] in ("output_rgba8", "output_bgra8"):
                w.state["rgba8"] = bool(s["value"]); w.state["bgra"] = bool(s["value"]) and s["name"] == "output_bgra8"
            elif s["op"] == "instances":
                w.state.update(count=s["count"], source=s["source"], time=s["time"])
            elif s["op"] == "materials":
                w.state["materials"] = s["which"]
            elif s["op"] == "types":
                w.state["types"] = s["which"]
            elif s["op"] == "sky":
                w.state["sky"] = (s["w"], s["h"])
        assert w.state == hs.BASE, (name, w.state)
    # the sizes: one pixel count with W and H swapped, partial tiles on both edges, a shard of 0 rows
    (sw, sh), (tw, th), (mw, mh) = hs.SIZES["small"], hs.SIZES["tall"], hs.SIZES["mid"]
    assert (sw, sh) == (th, tw) and sw != sh and mw % 8 and mh % 8
    empty = [s for s in steps if s["op"] == "empty_shard"]
    assert empty and all(tiling.shard_rows(sh, s["band"], s["shard"], s["n"]) == 0 for s in empty)
    assert any(s["op"] == "instances" and s["count"] > 32 for s in steps)            # past entry_max_instances and RT_LDS_INSTANCES
    assert any(s["op"] == "shards" and s["band"] % 8 for s in steps)                 # the coverage mask goes off (enqueue_frame's condition)


def mirror_world(ctx=None):
    """track B's scene: a mirror cube that fills the view (every primary sample makes one secondary ray), a diffuse cube behind the
    camera that the mirror shows"""
    def xf(s, t):
        return np.array([s, 0, 0, t[0], 0, s, 0, t[1], 0, 0, s, t[2]], np.float32)
    inst = np.asarray([host.make_instance(xf(10.0, (0, 0, 0)), 0, 0), host.make_instance(xf(1.5, (3, 1, 25)), 1, 1)], INSTANCE_DTYPE)
    g = host.SceneGeometry([CUBE, CUBE])
    u = host.default_uniforms(max_bounce_count=1, samples_per_pixel=hs.LARGE_SPP, center_object_type=1, orbiting_object_type=0,
                              orbiting_object_primitive_offset=g.orbiting_primitive_offset, orbiting_object_vertex_offset=g.orbiting_vertex_offset)
    return scenes.ScenePair([CUBE, CUBE], inst, u, sky=scenes.synthetic_skybox(16), ctx=ctx)


def track_b_uniforms(sp, name, depth):
    u = sp.uniforms.copy()
    u[0]["max_bounce_count"] = depth
    u[0]["samples_per_pixel"] = hs.track_b_frame(name)[2]
    return u


def test_track_b_large_frame_is_past_the_tail_threshold():
    """at depth 1 the oracle's secondary rays ARE the bounce-1 queue: at least 1.5 x TAIL_MAX_RAYS, so k_tail does not take bounce 1 of
    a large frame by itself — only a stale hint from a tiny frame sends it there; the tiny frame stays far below"""
    assert hs.tail_max_rays() == 16384
    sp = mirror_world()
    W, H, spp = hs.track_b_frame("large")
    sp.orc.set_uniforms(track_b_uniforms(sp, "large", 1).tobytes())
    rc = sp.orc.render(W, H, threads=ORACLE_THREADS)[1]
    print("track B large frame %d x %d spp %d: %d secondary rays, %.3f x TAIL_MAX_RAYS" % (W, H, spp, rc[1], rc[1] / hs.tail_max_rays()))
    assert rc[1] >= hs.TAIL_MAX_RAYS_MARGIN * hs.tail_max_rays() and rc[0] == W * H * spp
    w, h, s1 = hs.track_b_frame("tiny")
    sp.orc.set_uniforms(track_b_uniforms(sp, "tiny", 1).tobytes())
    assert 0 < sp.orc.render(w, h)[1][1] <= w * h * s1 < hs.tail_max_rays() // 16
    seq = [n for n, _ in hs.TRACK_B]
    assert seq[:4] == ["tiny", "large", "tiny", "large"] and ("large", 0) in hs.TRACK_B and hs.TRACK_B_SLOTS >= 3
    fam = hs.track_b_family()
    assert all(len({n for n, _ in phase}) == 2 for phase in fam)                     # tiny and large in flight together


def test_track_c_has_more_keys_than_the_cache_and_evicts_under_a_pending_frame():
    cap = hs.max_jitter_tables()
    assert len(set(hs.TRACK_C_KEYS)) == len(hs.TRACK_C_KEYS) == 11 > cap == 8
    assert all(W <= 48 and H <= 32 for W, H, *_ in hs.TRACK_C_KEYS)
    used = {k for _, k, _ in hs.TRACK_C}
    assert used == set(range(len(hs.TRACK_C_KEYS)))
    for slot, k, how in hs.TRACK_C:
        W, H, spp, band, shard, n = hs.TRACK_C_KEYS[k]
        assert 0 <= slot < hs.TRACK_C_SLOTS and tiling.shard_rows(H, band, shard, n) > 0
        assert how == "sync" or (band, shard, n) == (H, 0, 1)                         # trace_async renders full frames
    ev = hs.simulate_jitter_cache(hs.TRACK_C, hs.TRACK_C_KEYS, cap)
    assert len(ev) >= 4
    assert ev[0][1] == 0                                                              # the first key is evicted ...
    first_again = min(i for i, (_, k, _) in enumerate(hs.TRACK_C) if k == 0 and i > 0)
    assert ev[0][0] < first_again                                                     # ... before the script returns to it
    under = [e for e in ev if e[2]]
    assert len(under) >= 3 and all(hs.TRACK_C[e[0]][0] not in e[2] for e in under)    # caused by ANOTHER slot than the pending one
    pending = set()
    for slot, k, how in hs.TRACK_C:                                                   # every pending frame is collected, one per slot
        if how == "async":
            assert slot not in pending; pending.add(slot)
        elif how == "wait":
            pending.remove(slot)
        else:
            assert slot not in pending
    assert not pending


def test_track_d_sizes_and_kinds():
    assert hs.QUERY_SIZES == (5000, 37, 1, 5000) and hs.RAY_HITS_K[:3] == (1, 16, 3) and hs.POINT_HITS_K[:3] == (16, 0, 4)
    assert len(hs.RAY_HITS_K) == len(hs.POINT_HITS_K) == len(hs.QUERY_SIZES) and len(set(hs.QUERY_KINDS)) == 15


# ---- GPU: track A -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("script", hs.TRACK_A_SCRIPTS)
def test_track_a_one_context_every_kind_of_change(script):
    """caught: max_bounce_count 70 was accepted although the library's own message and csrc/rt_device.h give 69 as the limit"""
    t0 = time.time()
    steps = hs.track_a(script)
    w = World(RtContext(0), with_slot=True)
    try:
        run_script("A/" + script, steps, w.do)
    finally:
        w.close()
    print("track A %s: %d steps, %.2f s" % (script, len(steps), time.time() - t0))


# ---- GPU: track B -------------------------------------------------------------------------------------------------------------------------

class MirrorRefs:
    def __init__(self, sp):
        self.sp, self.refs = sp, {}

    def get(self, name, depth):
        W, H, _ = hs.track_b_frame(name)
        self.sp.orc.set_uniforms(track_b_uniforms(self.sp, name, depth).tobytes())
        if (name, depth) not in self.refs:
            self.refs[(name, depth)] = self.sp.orc.render(W, H, threads=ORACLE_THREADS)
        return self.refs[(name, depth)]

    def check(self, img, st, name, depth):
        W, H, _ = hs.track_b_frame(name)
        ref, rc = self.get(name, depth)
        assert_frame_equals_oracle(img, self.sp.orc, W, H, ref=ref)
        assert counts(st) == tuple(int(x) for x in rc), ("ray counts", counts(st), rc)


@pytest.mark.gpu
def test_track_b_hints_on_a_lone_context():
    t0 = time.time()
    ctx = RtContext(0)
    try:
        sp = mirror_world(ctx)
        refs = MirrorRefs(sp)

        def do(step):
            name, depth = step["frame"]
            W, H, _ = hs.track_b_frame(name)
            ctx.set_uniforms(track_b_uniforms(sp, name, depth))
            img, st = ctx.trace(W, H)
            refs.check(img, st, name, depth)
        steps = [dict(frame=f, desc="%s frame, depth %d, after %s" % (f[0], f[1], hs.TRACK_B[i - 1][0] if i else "nothing")) for i, f in enumerate(hs.TRACK_B)]
        run_script("B/lone", steps, do)
    finally:
        ctx.close()
    print("track B lone: %d steps, %.2f s" % (len(steps), time.time() - t0))


@pytest.mark.gpu
def test_track_b_hints_on_a_family_of_four():
    t0 = time.time()
    root = RtContext(0)
    slots = [root]
    try:
        sp = mirror_world(root)
        refs = MirrorRefs(sp)
        slots += [root.frame_slot() for _ in range(hs.TRACK_B_SLOTS - 1)]
        for s in slots[1:]:
            s.set_instances(sp.instances)

        def do(step):
            for s, (name, depth) in zip(slots, step["phase"]):     # all four in flight, tiny and large interleaved
                s.set_uniforms(track_b_uniforms(sp, name, depth))
                s.trace_async(*hs.track_b_frame(name)[:2])
            for k, (s, (name, depth)) in enumerate(zip(slots, step["phase"])):
                img, st = s.trace_wait()
                try:
                    refs.check(img, st, name, depth)
                except AssertionError as e:
                    raise AssertionError("slot %d (%s, depth %d): %s" % (k, name, depth, e)) from e
        steps = [dict(phase=p, desc="phase %d: %s" % (i, ", ".join("%s/d%d" % f for f in p))) for i, p in enumerate(hs.track_b_family())]
        run_script("B/family", steps, do)
    finally:
        for s in reversed(slots[1:]):
            s.close()
        root.close()
    print("track B family of %d: %d steps of %d frames, %.2f s" % (hs.TRACK_B_SLOTS, len(steps), hs.TRACK_B_SLOTS, time.time() - t0))


# ---- GPU: track C -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_track_c_jitter_tables_are_evicted_and_rebuilt():
    import torch
    t0 = time.time()
    w = World(RtContext(0))
    slots = [w.ctx]
    try:
        slots += [w.ctx.frame_slot() for _ in range(hs.TRACK_C_SLOTS - 1)]
        for s in slots[1:]:
            s.set_instances(instance_records(2, 0.0))
        pending = {}

        def do(step):
            slot, k, how = step["c"]
            W, H, spp, band, shard, n = hs.TRACK_C_KEYS[k]
            c = slots[slot]
            w.state.update(spp=spp)
            if how == "wait":
                img, st = c.trace_wait()
                assert pending.pop(slot) == k
                w.check(img, counts(st), W, H)
                return
            c.set_uniforms(w.uniforms())
            if how == "async":
                c.trace_async(W, H)
                pending[slot] = k
            elif (band, shard, n) == (H, 0, 1):
                img, st = c.trace(W, H)
                w.check(img, counts(st), W, H)
            else:
                rows = tiling.shard_row_map(H, band, shard, n)
                bands = [(int(y), int(min(y + band, H))) for y in range(shard * band, H, n * band)]
                ref, rc = w.reference(W, H, rows=bands)
                buf = torch.zeros((len(rows), W, 4), dtype=torch.float32, device="cuda:0")
                torch.cuda.synchronize()
                c.trace_shard(W, H, band, shard, n, buf.data_ptr(), buf.numel() * 4, stream_ptr())
                c.synchronize()
                st = c.stats()
                full = ref.copy()
                full[rows] = buf.cpu().numpy()
                for y0, y1 in bands:
                    assert_frame_equals_oracle(full, w.orc, W, H, y0=y0, y1=y1, ref=ref)
                assert counts(st) == tuple(int(x) for x in rc), ("ray counts", counts(st), rc)
        steps = [dict(c=c, desc="slot %d, key %d %s, %s" % (c[0], c[1], hs.TRACK_C_KEYS[c[1]], c[2])) for c in hs.TRACK_C]
        run_script("C", steps, do)
        assert not pending
    finally:
        for s in reversed(slots[1:]):
            s.close()
        w.ctx.close()
    print("track C: %d steps over %d keys, %.2f s" % (len(steps), len(hs.TRACK_C_KEYS), time.time() - t0))


# ---- GPU: track D -------------------------------------------------------------------------------------------------------------------------

def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def query_inputs(n, seed):
    """the records of every query kind for a round of n, about the origin where both of track D's scenes have surfaces"""
    rng = np.random.default_rng(seed)
    q = {}
    q["rays"] = scenes.random_rays(n, seed=seed + 1)
    q["any"] = q["rays"].copy(); q["any"][:, 7] = 25.0
    words = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & np.uint32(0xFF0003FB)   # (no terminate-on-first-hit: its answer depends on the tree)
    words[::5] = 0xFF000000
    q["words"] = words
    q["points"] = np.concatenate([rng.uniform(-3, 3, (n, 3)), np.where(np.arange(n) % 4 == 0, 1.0, np.inf)[:, None]], axis=1).astype(np.float32)
    c, h = rng.uniform(-2.5, 2.5, (n, 3)), 10 ** rng.uniform(-2, -0.3, (n, 3))
    boxes = np.zeros((n, 8), np.float32); boxes[:, 0:3] = c - h; boxes[:, 4:7] = c + h
    q["boxes"] = boxes
    a = rng.uniform(-2.5, 2.5, (n, 3))
    tris = np.zeros((n, 12), np.float32)
    tris[:, 0:3] = a; tris[:, 4:7] = a + rng.uniform(-0.4, 0.4, (n, 3)); tris[:, 8:11] = a + rng.uniform(-0.4, 0.4, (n, 3))
    tris[:, 3] = np.where(np.arange(n) % 3 == 0, 2.0, np.inf)
    q["tris"] = tris
    o = unit(rng.normal(size=(n, 3))) * 12.0
    sw = np.zeros((n, 8), np.float64)
    sw[:, 0:3] = o; sw[:, 3] = 10 ** rng.uniform(-2, -0.5, n); sw[:, 4:7] = unit(rng.uniform(-2, 2, (n, 3)) - o); sw[:, 7] = np.where(np.arange(n) % 3 == 0, np.inf, 30.0)
    q["sweeps"] = sw.astype(np.float32)
    p0 = rng.uniform(-3, 3, (n, 3))
    q["segs"] = api.capsule_records(p0, p0 + rng.uniform(-1, 1, (n, 3)), np.where(np.arange(n) % 4 == 1, 1.0, np.inf))
    q["shade"] = scenes.random_rays(2 * n, seed=seed + 2)      # two samples of n points
    return q


def to_device(q):
    import torch
    d = {k: torch.from_numpy(np.ascontiguousarray(v.view(np.int32) if v.dtype == np.uint32 else v)).to("cuda:0") for k, v in q.items()}
    torch.cuda.synchronize()
    return d


def call_kind(c, kind, d, i, stream=None):
    """one call of the kind over the device records d at position i of hs.QUERY_SIZES -> the result tensors, in a fixed order"""
    if kind == "intersect":
        r = c.intersect_device(d["rays"], attributes=True, stream=stream); return [r.hits, r.attr]
    if kind == "intersect_any":
        return [c.intersect_device(d["any"], any_hit=True, stream=stream).hits]
    if kind == "flags":
        r = c.intersect_device_flags(d["rays"], ray_flags=api.RAY_FLAG_CULL_BACK_FACING, words=d["words"], attributes=True, stream=stream); return [r.hits, r.attr]
    if kind == "ray_hits":
        r = c.intersect_device_hits(d["rays"], hs.RAY_HITS_K[i], attributes=True, counts=True, stream=stream); return [r.hits, r.attr, r.count]
    if kind == "closest_point":
        r = c.closest_point_device(d["points"], attributes=True, stream=stream); return [r.hits, r.attr]
    if kind == "point_hits":
        k = hs.POINT_HITS_K[i]
        r = c.closest_point_device_hits(d["points"], k, attributes=k > 0, counts=True, stream=stream); return [t for t in (r.hits, r.attr, r.count) if t is not None]
    if kind == "overlap_boxes":
        r = c.overlap_boxes_device(d["boxes"], max_ids=16, stream=stream); return [r.ids, r.count]
    if kind == "overlap_triangles":
        r = c.overlap_triangles_device(d["tris"], max_ids=16, stream=stream); return [r.ids, r.count]
    if kind == "sweep":
        r = c.sweep_spheres_device(d["sweeps"], attributes=True, stream=stream); return [r.hits, r.attr]
    if kind == "segment":                                      # attributes without params: the parameters go through the workspace's words
        r = c.closest_segment_device(d["segs"], attributes=True, params=False, stream=stream); return [r.hits, r.attr]
    if kind == "triangle":
        r = c.closest_triangle_device(d["tris"], attributes=True, params=False, stream=stream); return [r.hits, r.attr]
    if kind == "inside":
        r = c.point_inside_device(d["points"], n_dirs=3, counts=True, stream=stream); return [r.word, r.count]
    if kind == "signed_distance":                              # without an `inside` buffer: the vote words are the workspace's
        r = c.signed_distance_device(d["points"], n_dirs=3, attributes=True, stream=stream); return [r.hits, r.attr]
    if kind == "shade_library":                                # per-sample colours in the library's buffer
        return [c.shade_rays_device(d["shade"], samples=2, per_sample=False, points=True, stream=stream)[1]]
    if kind == "shade_caller":                                 # ... and in the caller's
        return list(c.shade_rays_device(d["shade"], samples=2, per_sample=True, points=True, stream=stream))
    raise ValueError(kind)


def host_copies(tensors):
    return [t.cpu().numpy() for t in tensors]


class QueryState:
    """what track D's context holds: the geometry, a refit of mesh 0, the instance records and their source; apply() is the shortest
    way a fresh context gets there"""

    def __init__(self, name, verts, idx, ranges, inst, source="host", refit=None, uniforms=None, sky=None):
        self.name, self.verts, self.idx, self.ranges, self.inst, self.source, self.refit = name, verts, idx, ranges, inst, source, refit
        self.uniforms, self.sky = uniforms, sky

    def set_instances(self, c):
        if self.source == "host":
            c.set_instances(self.inst)
        else:
            c.set_instances_device(device_records(self.inst))

    def refit_on(self, c):
        import torch
        t = torch.from_numpy(self.refit.reshape(-1, 6).copy()).to("cuda:0")
        torch.cuda.synchronize()
        c.refit_blas_device(0, t)

    def apply(self, c):
        c.upload_geometry(self.verts, self.idx, self.ranges)
        if self.refit is not None:
            c.set_instances(self.inst)                         # (a refit needs a linked scene)
            self.refit_on(c)
        self.set_instances(c)
        c.set_uniforms(self.uniforms)
        c.set_skybox(self.sky)

    def world_verts(self):
        v = self.verts.copy()
        if self.refit is not None:
            v[:len(self.refit)] = self.refit
        return v


def fresh_result(state, kind, d, i):
    import torch
    c = RtContext(0)
    try:
        state.apply(c)
        out = call_kind(c, kind, d, i)
        torch.cuda.synchronize()
        return host_copies(out)
    finally:
        c.close()


def anchor(state, kind, q, i, res):
    """the fresh context's result against the kind's CPU reference"""
    sc = cr.Scene(state.world_verts(), state.idx, state.ranges, state.inst)
    orc = oracle.OracleScene()
    orc.set_geometry(state.world_verts(), state.idx, state.ranges)
    orc.set_instances([state.inst[k].tobytes() for k in range(len(state.inst))])
    orc.set_uniforms(state.uniforms.tobytes())
    orc.set_skybox(state.sky)
    hits = lambda a: np.ascontiguousarray(a).view(HIT_DTYPE).reshape(a.shape[:-1])   # noqa: E731
    n = len(q["rays"])
    if kind == "intersect":
        assert_hits_equal_oracle(hits(res[0]), orc, q["rays"])
        o = orc.hit_attributes(hits(res[0]))
        assert np.array_equal(res[1][:, 0:3].view(np.uint32), o[:, 0:3].view(np.uint32)) and np.array_equal(res[1][:, 4:7].view(np.uint32), o[:, 3:6].view(np.uint32))
    elif kind == "intersect_any":                              # which blocker a walk meets first depends on the tree: blocked or not does not
        assert np.array_equal(hits(res[0])["inst"] >= 0, orc.intersect(q["any"], any_hit=True)["inst"] >= 0)
    elif kind == "flags":
        ref, kinds = orc.intersect_query(q["rays"], words=q["words"], ray_flags=api.RAY_FLAG_CULL_BACK_FACING)
        assert hits(res[0]).tobytes() == ref.tobytes() and np.array_equal(res[1][:, 7].view(np.uint32), kinds)
    elif kind == "ray_hits":
        orc.tri_counts = ir.tri_counts(state.ranges, state.inst)
        from tests.test_ray_query_hits import oracle_lists
        ref, kinds, cnt = oracle_lists(orc, q["rays"], None, 0, 0xFF, hs.RAY_HITS_K[i])
        assert hits(res[0]).tobytes() == ref.tobytes() and np.array_equal(res[2].view(np.uint32), cnt)
    elif kind == "closest_point":
        assert hits(res[0]).tobytes() == cr.brute32(sc, q["points"]).tobytes()
    elif kind == "point_hits":
        k = hs.POINT_HITS_K[i]
        ref, cnt = chr_.brute32_k(sc, q["points"], k)
        assert np.array_equal(res[-1].view(np.uint32), cnt)
        if k:
            assert hits(res[0]).tobytes() == ref.tobytes()
    elif kind in ("overlap_boxes", "overlap_triangles"):
        mod, recs = (orf, q["boxes"]) if kind == "overlap_boxes" else (tor, q["tris"])
        cnt, ids = mod.brute32(sc, recs, max_ids=16, tris=orf.Triangles(sc))
        assert res[1].astype(cnt.dtype).tobytes() == cnt.tobytes() and res[0].astype(ids.dtype).tobytes() == np.ascontiguousarray(ids[:, :16]).tobytes()
    elif kind == "sweep":
        assert hits(res[0]).tobytes() == sr.brute32(sc, q["sweeps"]).tobytes()
    elif kind == "segment":
        assert hits(res[0]).tobytes() == sgr.brute32(sc, q["segs"])[0].tobytes()
    elif kind == "triangle":
        assert hits(res[0]).tobytes() == tdr.brute32(sc, q["tris"])[0].tobytes()
    elif kind in ("inside", "signed_distance"):
        cnt = ir.oracle_counts(orc, ir.tri_counts(state.ranges, state.inst), q["points"], 3)
        if kind == "inside":
            assert np.array_equal(res[1].view(np.uint32), cnt) and np.array_equal(res[0].view(np.uint32), ir.words(cnt, 3, True))
        else:
            from tests.consumers import sign_split
            raw, sign = sign_split(hits(res[0]))
            craw, csign = sign_split(cr.brute32(sc, q["points"]))
            assert np.array_equal(raw, craw) and np.array_equal(sign, csign | (ir.words(cnt, 3, True) & 1))
    elif kind in ("shade_library", "shade_caller"):
        s = shade_samples(orc, q["shade"], n, int(state.uniforms[0]["max_bounce_count"]))
        assert np.array_equal(res[-1].view(np.uint32), average_points(s, n, 2).view(np.uint32))
        if kind == "shade_caller":
            assert np.array_equal(res[0].view(np.uint32), s.view(np.uint32))
    else:
        raise ValueError(kind)


@pytest.mark.gpu
def test_track_d_query_and_shading_workspace():
    import torch
    t0 = time.time()
    rng = np.random.default_rng(hs.TRACK_D_SEED)
    g = host.SceneGeometry([TEAPOT, CUBE])
    u = host.default_uniforms(max_bounce_count=2, samples_per_pixel=2, center_object_type=1, orbiting_object_type=0,
                              orbiting_object_primitive_offset=g.orbiting_primitive_offset, orbiting_object_vertex_offset=g.orbiting_vertex_offset)
    sky = scenes.synthetic_skybox(32)
    first = QueryState("teapot + cube", g.verts, g.idx, g.ranges, instance_records(2, 0.0), uniforms=u, sky=sky)
    cv, ci = scenes.corridor(hs.CORRIDOR_SQUARES)
    cv = cv.copy(); cv[:, 2] += 20.0                            # squares from z = 20 down to z = -21: the records about the origin meet them
    ident = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    turned = ingest.glm_to_vulkan(ingest.mat_translate(ingest.mat_rotate_y(ingest.mat_identity(), np.float32(1.2)), (0.5, 0.0, 0.0)))
    deep = QueryState("corridor", cv.reshape(-1), ci, [(0, 0, len(ci) // 3)],
                      np.asarray([host.make_instance(ident, 0, 0), host.make_instance(turned, 1, 0)], INSTANCE_DTYPE), uniforms=u, sky=sky)
    span = 6 * (int(g.idx[:3 * g.ranges[0][2]].max()) + 1)
    bent = g.verts[:span].copy().reshape(-1, 6)
    bent[:, :3] += (np.float32(0.15) * np.sin(np.float32(2.5) * bent[:, [1, 2, 0]] + np.float32(0.7))).astype(np.float32)
    refitted = QueryState("teapot refitted", g.verts, g.idx, g.ranges, first.inst, refit=bent.reshape(-1), uniforms=u, sky=sky)
    moved = QueryState("device instances", g.verts, g.idx, g.ranges, instance_records(2, 0.4), source="device", refit=bent.reshape(-1), uniforms=u, sky=sky)

    inputs = {n: query_inputs(n, hs.TRACK_D_SEED + n) for n in set(hs.QUERY_SIZES)}
    dev = {n: to_device(q) for n, q in inputs.items()}
    fresh, anchored, n_steps = {}, set(), [0]
    ctx = RtContext(0)
    side = torch.cuda.Stream()
    frame_orc = scenes.two_object_scene(TEAPOT, CUBE, 1, 0, 2, 2, sky=sky)
    try:
        first.apply(ctx)

        def round_of(state, i, order, pending_frame):
            """every kind once at size i on the long-lived context, back to back on alternating streams; then each against a fresh context"""
            n = hs.QUERY_SIZES[i]
            if pending_frame:
                ctx.trace_async(70, 36)
            got = {}
            for j, kind in enumerate(order):
                got[kind] = call_kind(ctx, kind, dev[n], i, stream=side if j % 2 else None)
            torch.cuda.synchronize()
            if pending_frame:
                img, st = ctx.trace_wait()
                ref, rc = frame_orc.orc.render(70, 36)
                assert_frame_equals_oracle(img, frame_orc.orc, 70, 36, ref=ref)
                assert counts(st) == tuple(int(x) for x in rc)
            for kind in order:
                k = (hs.RAY_HITS_K[i] if kind == "ray_hits" else hs.POINT_HITS_K[i] if kind == "point_hits" else 0)
                key = (state.name, kind, n, k)
                if key not in fresh:
                    fresh[key] = fresh_result(state, kind, dev[n], i)
                    if state is first and n <= hs.SHORT_ROUND_N and (kind, k) not in anchored:
                        anchor(state, kind, inputs[n], i, fresh[key])
                        anchored.add((kind, k))
                res = host_copies(got[kind])
                n_steps[0] += 1
                assert len(res) == len(fresh[key])
                for a, b in zip(res, fresh[key]):
                    assert a.shape == b.shape and a.tobytes() == b.tobytes(), \
                        "%s, n %d, on %s: %d of %d bytes differ from the fresh context's" % (kind, n, state.name, int((a.view(np.uint8) != b.view(np.uint8)).sum()), a.nbytes)

        def do(step):
            if step.get("change") == "deeper geometry":
                ctx.upload_geometry(deep.verts, deep.idx, deep.ranges); deep.set_instances(ctx)
            elif step.get("change") == "first geometry again":
                ctx.upload_geometry(first.verts, first.idx, first.ranges); first.set_instances(ctx)
            elif step.get("change") == "refit_blas_device":
                refitted.refit_on(ctx); refitted.set_instances(ctx)
            elif step.get("change") == "set_instances_device":
                moved.set_instances(ctx)
            order = [hs.QUERY_KINDS[k] for k in rng.permutation(len(hs.QUERY_KINDS))]
            round_of(step["state"], step["i"], order, step.get("pending", False))
        steps = [dict(state=first, i=i, pending=i % 2 == 1, desc="every kind at n = %d%s" % (n, " beside a pending frame" if i % 2 else ""))
                 for i, n in enumerate(hs.QUERY_SIZES)]
        short = hs.QUERY_SIZES.index(hs.SHORT_ROUND_N)
        for change, state in zip(hs.TRACK_D_CHANGES, (deep, first, refitted, moved)):
            steps.append(dict(state=state, i=short, change=change, desc="a short round after: " + change))
        run_script("D", steps, do)
        assert {k for k, _ in anchored} == set(hs.QUERY_KINDS), sorted(set(hs.QUERY_KINDS) - {k for k, _ in anchored})
    finally:
        ctx.close()
    print("track D: %d rounds, %d results compared with %d fresh contexts, %d anchored to CPU references, %.2f s"
          % (len(steps), n_steps[0], len(fresh), len(anchored), time.time() - t0))


# ---- GPU: track E -------------------------------------------------------------------------------------------------------------------------

def scene_b():
    """three meshes (teapot, cube, a corridor of 4096 squares: a deeper tree) and four instances"""
    cv, ci = scenes.corridor(hs.CORRIDOR_SQUARES, spacing=0.002)
    cv = cv.copy()
    cv[:, 0:3] *= np.float32(0.25)
    cv[:, 0] -= 5.0; cv[:, 2] += 2.0
    g = host.SceneGeometry([TEAPOT, CUBE])
    verts = np.concatenate([g.verts, cv.reshape(-1)])
    idx = np.concatenate([g.idx, ci])
    ranges = list(g.ranges) + [(len(g.verts), len(g.idx), len(ci) // 3)]
    ident = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    base = instance_records(2, 0.2)
    up = np.array([1, 0, 0, 3.0, 0, 1, 0, 2.5, 0, 0, 1, 1.0], np.float32)
    inst = np.asarray([base[0], base[1], host.make_instance(ident, 1, 2), host.make_instance(up, 1, 1)], INSTANCE_DTYPE)
    return verts, idx, ranges, inst


@pytest.mark.gpu
def test_track_e_geometry_replaced_under_a_family():
    """rt_upload_geometry removes the material table (include/rt_api.h, rt_set_materials): after the re-upload the frames are those of a
    scene without a table, and the old table is refused as a whole until it is set again for the new index buffer"""
    t0 = time.time()
    W, H = hs.SIZES["mid"]
    w = World(RtContext(0))
    root = w.ctx
    slots = [root]
    n_steps = 0
    try:
        slots += [root.frame_slot() for _ in range(2)]
        for s in slots[1:]:
            s.set_instances(instance_records(2, 0.0)); s.set_uniforms(w.uniforms())
        for s in slots:
            img, st = s.trace(W, H); w.check(img, counts(st), W, H); n_steps += 1
        # scene B through a slot, not the root
        verts, idx, ranges, inst = scene_b()
        orc_b = oracle.OracleScene()
        orc_b.set_geometry(verts, idx, ranges)
        orc_b.set_instances([inst[i].tobytes() for i in range(len(inst))])
        orc_b.set_uniforms(w.uniforms().tobytes())
        orc_b.set_skybox(sky_faces(*w.state["sky"]))
        ref_b, rc_b = orc_b.render(W, H, threads=ORACLE_THREADS)
        assert rc_b[1] > 0 and rc_b[2] > 0
        w.op_materials(dict(which="A"))
        img, st = slots[2].trace(W, H); w.check(img, counts(st), W, H); n_steps += 1
        slots[1].upload_geometry(verts, idx, ranges)
        for k, s in enumerate(slots):
            expect_error(lambda: s.trace(W, H), RT_ERR_NOT_READY, s, "slot %d before its set_instances" % k)
        order = (2, 0, 1)
        for pos, k in enumerate(order):
            slots[k].set_instances(inst)
            for j in order[pos + 1:]:                                    # one member's set_instances does not ready the others
                expect_error(lambda: slots[j].trace(W, H), RT_ERR_NOT_READY, slots[j], "slot %d, whose instances are not set yet" % j)
            img, st = slots[k].trace(W, H)
            assert_frame_equals_oracle(img, orc_b, W, H, ref=ref_b)      # (no material table: the upload removed it)
            assert counts(st) == tuple(int(x) for x in rc_b), ("slot %d on scene B" % k, counts(st), rc_b)
            n_steps += 1
        # the old table belongs to the old index buffer: one id per triangle of the NEW one is asked for
        expect_error(lambda: root.set_materials(*w.tables["A"]), RT_ERR_INVALID_ARGUMENT, root, "scene A's material ids on scene B")
        img, st = root.trace(W, H)
        assert_frame_equals_oracle(img, orc_b, W, H, ref=ref_b); n_steps += 1
        # back to A, through the root; the table is set again and shades
        w.state["materials"] = None
        root.upload_geometry(w.geom.verts, w.geom.idx, w.geom.ranges)
        for s in slots:
            expect_error(lambda: s.trace(W, H), RT_ERR_NOT_READY, s, "after the second re-upload")
            s.set_instances(instance_records(2, 0.0))
            img, st = s.trace(W, H); w.check(img, counts(st), W, H); n_steps += 1
        w.op_materials(dict(which="A"))
        for s in slots:
            img, st = s.trace(W, H); w.check(img, counts(st), W, H); n_steps += 1
    finally:
        for s in reversed(slots[1:]):
            s.close()
        root.close()
    print("track E re-upload: %d frames and 10 refused calls, %.2f s" % (n_steps, time.time() - t0))


@pytest.mark.gpu
def test_track_e_destroy_order_and_slot_limit():
    t0 = time.time()
    W, H = hs.SIZES["mid"]
    w = World(RtContext(0))
    root = w.ctx
    a = root.frame_slot(); b = root.frame_slot()
    live = [a, b]
    try:
        for s in live:
            s.set_instances(instance_records(2, 0.0)); s.set_uniforms(w.uniforms())
        a.trace_async(W, H)
        root.close()                                            # the root first, with a frame pending on a slot
        img, st = a.trace_wait()
        w.check(img, counts(st), W, H)
        img, st = b.trace(W, H)
        w.check(img, counts(st), W, H)
        b.trace_async(W, H)
        a.close(); live.remove(a)
        img, st = b.trace_wait()
        w.check(img, counts(st), W, H)
        # 16 contexts per scene: b and 15 more; the 17th is refused; destroyed and created again
        for rnd in range(2):
            more = []
            try:
                more = [b.frame_slot() for _ in range(15)]
                with pytest.raises(RtError) as e:
                    b.frame_slot()
                assert e.value.code == RT_ERR_INVALID_ARGUMENT and "16" in str(e.value)
            finally:
                for s in reversed(more):
                    s.close()
        new = b.frame_slot(); live.append(new)
        new.set_instances(instance_records(2, 0.0)); new.set_uniforms(w.uniforms())
        img, st = new.trace(W, H)
        w.check(img, counts(st), W, H)
        img, st = b.trace(W, H)
        w.check(img, counts(st), W, H)
    finally:
        for s in reversed(live):
            s.close()
        root.close()
    print("track E destroy order: 6 frames, 2 x 15 slots, %.2f s" % (time.time() - t0))


@pytest.mark.gpu
def test_track_e_device_memory_returns_after_destroy():
    """30 times: create, upload, a 70 x 36 frame, a query of 5000 rays, destroy.  Free device memory after cycle 30 is below that
    after cycle 2 by less than one live context's footprint (measured in cycle 2): a buffer leaked per context would cost 28 of them.
    The query runs on ONE stream of the caller's, made before the loop.  On torch's default stream every RtContext takes a side stream
    of its own from torch's pool (api._on_stream), and torch creates the streams of that pool on first use and never destroys them:
    measured on an MI355X that way, 1 MiB per cycle (29 360 128 bytes over 28 cycles, against a footprint of 123 731 968), none of it the
    library's: the same cycles without the query drop 0 bytes, and so do 28 bare hipStreamCreate / hipStreamDestroy pairs."""
    import torch
    t0 = time.time()
    W, H = hs.SIZES["mid"]
    geom = host.SceneGeometry([TEAPOT, CUBE])
    u = World().uniforms()
    inst, sky = instance_records(2, 0.0), sky_faces(64, 64)
    rays = torch.from_numpy(scenes.random_rays(5000, seed=9)).to("cuda:0")
    out = (torch.empty((5000, 5), dtype=torch.int32, device="cuda:0"), None)
    side = torch.cuda.Stream()

    def free():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info(0)[0]
    first_img, first_hits, footprint, after2 = None, None, None, None
    for cycle in range(1, 31):
        before = free()
        c = RtContext(0)
        try:
            c.upload_geometry(geom.verts, geom.idx, geom.ranges)
            c.set_instances(inst); c.set_uniforms(u); c.set_skybox(sky)
            img, _ = c.trace(W, H)
            c.intersect_device(rays, out=out, stream=side)
            torch.cuda.synchronize()
            hits = out[0].cpu().numpy().copy()
            if cycle == 2:
                footprint = before - free()
        finally:
            c.close()
        if first_img is None:
            first_img, first_hits = img, hits
        assert img.tobytes() == first_img.tobytes() and hits.tobytes() == first_hits.tobytes(), "cycle %d" % cycle
        if cycle == 2:
            after2 = free()
    after30 = free()
    print("track E device memory: one live context %d bytes; free after cycle 2 %d, after cycle 30 %d: drop %d bytes (%.2f s)"
          % (footprint, after2, after30, after2 - after30, time.time() - t0))
    assert footprint > 0
    assert after2 - after30 < footprint, (after2 - after30, footprint)
