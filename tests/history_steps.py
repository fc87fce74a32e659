"""The scripts of tests/test_context_history.py, as data: what one long-lived context family is taken through, step by step.

A step is a dict: "op" (what the interpreter of tests/test_context_history.py does), "desc" (the words a failure message carries), the
operands of the op, and optionally "tag", the name of a required transition the step stands for.  The scripts hold no GPU call, so the
CPU tests can check their premises: that every required transition is there (track A), that the large frame's bounce-1 queue is past
TAIL_MAX_RAYS (track B), that the keys of track C are more than the jitter-table cache holds and that an eviction happens while a
frame is pending.

Track A is a list of TRANSITIONS.  Every transition starts from the BASE state and ends in it, so any order of them is a valid life of
a context: the fixed script is the list as written, and PERMUTATION_SEEDS name two shuffles of it."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- frame sizes --------------------------------------------------------------------------------------------------------------------
SIZES = {"small": (40, 24),      # whole 8x8 tiles
         "tall": (24, 40),       # small with W and H swapped: the same pixel count
         "mid": (70, 36),        # partial tiles on both edges
         "large": (136, 92)}     # track B's large frame (LARGE below)
BASE = dict(size="small", spp=2, depth=2, light=None, count=2, source="host", time=0.0, materials=None, types=None, sky=(64, 64),
            rgba8=False, bgra=False)
LIGHT_MOVED = (-4.0, 6.0, 3.0)
TUNABLES = ("pixel_beams", "fused_shade", "entry_points", "primary_cover", "jitter_table", "dead_shadow_rays")
REJECTS = ("spp0", "depth70", "update_count", "uniforms_in_batch")
PERMUTATION_SEEDS = (20261, 20262)


def S(op, desc, tag=None, **kw):
    step = dict(op=op, desc=desc, **kw)
    if tag:
        step["tag"] = tag
    return step


def frame(desc, size=None, tag=None, mode="trace"):
    return S("frame", desc, tag, size=size, mode=mode)


def _tunable(name, size):
    return [S("param", "%s off" % name, name=name, value=0), frame("frame with %s off" % name, size, "tunable:" + name),
            S("param", "%s back on" % name, name=name, value=1), frame("frame with %s on again" % name, size)]


TRANSITIONS = [
    ("frame size", [
        frame("small frame", "small"),
        frame("large frame after small", "large", "size:small>large"),
        frame("small frame after large", "small", "size:large>small"),
        frame("large frame again", "large"),
        frame("small frame with W and H swapped", "tall", "size:swap"),
        frame("small frame after the swapped one", "small"),
        S("empty_shard", "a shard of 0 rows between two frames", "size:empty", band=8, n=4, shard=3),
        frame("small frame after the empty shard", "small"),
        frame("mid frame (partial tiles)", "mid"),
        frame("back to the small frame", "small")]),
    ("spp and bounce depth", [
        S("uniforms", "spp 1", spp=1), frame("frame at spp 1", "mid"),
        S("uniforms", "spp 5", spp=5), frame("frame at spp 5 after 1", "mid", "spp:1>5"),
        S("uniforms", "spp 2", spp=2), frame("frame at spp 2 after 5", "mid", "spp:5>2"),
        S("uniforms", "depth 0", depth=0), frame("frame at depth 0", "small"),
        S("uniforms", "depth 4", depth=4), frame("frame at depth 4 after 0", "small", "depth:0>4"),
        S("uniforms", "depth 0", depth=0), frame("frame at depth 0 after 4", "small", "depth:4>0"),
        S("uniforms", "depth 63 (the reference's default)", depth=63), frame("frame at depth 63", "small", "depth:63"),
        S("uniforms", "depth 3, spp 3", depth=3, spp=3), frame("frame at depth 3, spp 3", "mid"),
        S("uniforms", "back to the base uniforms", depth=BASE["depth"], spp=BASE["spp"]), frame("base frame", "small")]),
    ("shard layout", [
        frame("full frame", "mid"),
        S("shards", "shards of band_rows 8", "shards:8", band=8, n=3),
        S("shards", "shards of band_rows 4 (no coverage mask)", "shards:4", band=4, n=2),
        frame("full frame after the shards", "mid", "shards:full"),
        S("shards", "shards of band_rows 8 again", band=8, n=2),
        frame("base frame", "small")]),
    ("output format", [
        S("param", "output_rgba8 1", name="output_rgba8", value=1), frame("RGBA8 frame", "mid", "format:rgba8"),
        S("param", "output_bgra8 1", name="output_bgra8", value=1), frame("BGRA8 frame", "small", "format:bgra8"),
        S("param", "output_bgra8 0 (both off)", name="output_bgra8", value=0), frame("RGBA32F frame again", "mid", "format:rgba32f"),
        frame("base frame", "small")]),
    ("instance source and count", [
        S("instances", "host records, built", source="host", count=2, update=False, time=0.1), frame("host instances", "small"),
        S("instances", "host records moved, update", "inst:host_update", source="host", count=2, update=True, time=0.3), frame("host instances moved", "small"),
        S("instances", "device records, built", "inst:host>device", source="device", count=2, update=False, time=0.3), frame("device instances", "small"),
        S("instances", "device records moved, update", "inst:device_update", source="device", count=2, update=True, time=0.5), frame("device instances moved", "mid"),
        S("instances", "host records again, built", "inst:device>host", source="host", count=2, update=False, time=0.5), frame("host instances after device", "small"),
        S("instances", "40 host records", "inst:2>40", source="host", count=40, update=False, time=0.5), frame("40 instances", "mid"),
        S("instances", "40 host records moved, update", source="host", count=40, update=True, time=0.7), frame("40 instances moved", "mid"),
        S("instances", "40 device records", source="device", count=40, update=False, time=0.7), frame("40 device instances", "small"),
        S("instances", "2 device records after 40", "inst:40>2", source="device", count=2, update=False, time=0.2), frame("2 device instances after 40", "mid"),
        S("instances", "base instances", source="host", count=2, update=False, time=0.0), frame("base frame", "small")]),
    ("batches", [
        S("batch", "batch of 3 frames", "batch:3", K=3, size="small"),
        S("instances", "single frames after the batch", "batch:single", source="host", count=2, update=False, time=0.0), frame("single frame after a batch of 3", "small"),
        S("batch", "batch of 2 frames", "batch:2", K=2, size="mid"),
        S("batch", "batch of 3 frames, update", K=3, size="small", update=True),
        S("instances", "base instances", source="host", count=2, update=False, time=0.0), frame("base frame", "small")]),
    ("shading tables", [
        S("materials", "material table A (4 materials)", "materials:A", which="A"), frame("frame with table A", "mid"),
        S("materials", "no material table", "materials:none", which=None), frame("frame without a table", "mid"),
        S("materials", "material table B (2 materials)", "materials:B", which="B"), frame("frame with table B", "small"),
        S("types", "instance types set", "types:list", which="mixed"), frame("frame with instance types and table B", "mid"),
        S("materials", "no material table", which=None), frame("frame with instance types", "small"),
        S("types", "instance types removed", "types:empty", which=None), frame("base frame", "small")]),
    ("sky", [
        S("sky", "sky 16 x 16", "sky:64>16", w=16, h=16), frame("frame under the 16 x 16 sky", "mid"),
        S("sky", "sky 32 x 16 (not square)", "sky:nonsquare", w=32, h=16), frame("frame under the 32 x 16 sky", "mid"),
        S("sky", "sky 64 x 64", "sky:>64", w=64, h=64), frame("base frame", "small")]),
    ("light", [
        frame("light held, frame 1", "mid"), frame("light held, frame 2", "mid"), frame("light held, frame 3 (kept records in use)", "mid", "light:kept"),
        S("param", "shadow_entry 0", "shadow_entry:2>0", name="shadow_entry", value=0), frame("frame with shadow_entry 0", "mid"),
        S("uniforms", "light moved", light=LIGHT_MOVED), frame("frame with the light moved", "mid", "light:moved"),
        S("param", "shadow_entry 2", "shadow_entry:0>2", name="shadow_entry", value=2), frame("moved light, shadow_entry 2, frame 1", "mid"),
        frame("moved light, shadow_entry 2, frame 2", "mid"),
        S("uniforms", "light moved back", light=None), frame("frame with the light back", "mid", "light:back"),
        frame("light back, frame 2", "mid"), frame("light back, frame 3", "small"), frame("base frame", "small")]),
    ("tunables", sum([_tunable(name, "mid" if k % 2 else "small") for k, name in enumerate(TUNABLES)], []) + [frame("base frame", "small")]),
    ("counting", [
        frame("plain frame", "mid"), frame("counting frame", "mid", "counting", mode="counting"), frame("plain frame after counting", "mid"),
        frame("base frame", "small")]),
    ("rejected calls", [S("reject", "rejected: %s" % k, "reject:" + k, kind=k, size="mid" if i % 2 else "small") for i, k in enumerate(REJECTS)]
     + [frame("base frame", "small")]),
]

REQUIRED_TAGS = frozenset(
    ["size:small>large", "size:large>small", "size:swap", "size:empty", "spp:1>5", "spp:5>2", "depth:0>4", "depth:4>0", "depth:63",
     "shards:8", "shards:4", "shards:full", "format:rgba8", "format:bgra8", "format:rgba32f",
     "inst:host_update", "inst:host>device", "inst:device_update", "inst:device>host", "inst:2>40", "inst:40>2",
     "batch:3", "batch:single", "batch:2", "materials:A", "materials:none", "materials:B", "types:list", "types:empty",
     "sky:64>16", "sky:nonsquare", "sky:>64", "light:kept", "light:moved", "light:back", "shadow_entry:2>0", "shadow_entry:0>2", "counting"]
    + ["tunable:" + n for n in TUNABLES] + ["reject:" + k for k in REJECTS])

TRACK_A_SCRIPTS = ("fixed",) + tuple("seed%d" % s for s in PERMUTATION_SEEDS)


def track_a(script):
    """the steps of a track A script: "fixed", or "seed<N>" for the transitions shuffled by numpy's default_rng(N)"""
    order = list(range(len(TRANSITIONS)))
    if script != "fixed":
        seed = int(script[len("seed"):])
        assert seed in PERMUTATION_SEEDS
        order = [int(k) for k in np.random.default_rng(seed).permutation(len(TRANSITIONS))]
    return [dict(st, transition=TRANSITIONS[k][0]) for k in order for st in TRANSITIONS[k][1]]


# ---- track B: hints from the previous frame -----------------------------------------------------------------------------------------
TAIL_MAX_RAYS_MARGIN = 1.5
LARGE = SIZES["large"]           # a mirror cube fills the view: every primary sample makes one secondary ray, 136 * 92 * 2 = 25024
TINY = (8, 8)
LARGE_SPP, TINY_SPP = 2, 1
# (frame, max_bounce_count): tiny -> large -> tiny -> large, then large without the hinted bounce (depth 0), then with bounces again
TRACK_B = [("tiny", 1), ("large", 1), ("tiny", 1), ("large", 1), ("large", 0), ("large", 3), ("tiny", 3), ("large", 1)]
TRACK_B_SLOTS = 4                # >= 3 members: the grid caps and the hinted k_tail grid are in force


def track_b_frame(name):
    """(W, H, spp) of a track B frame"""
    return (LARGE + (LARGE_SPP,)) if name == "large" else (TINY + (TINY_SPP,))


def track_b_family():
    """per phase, what each of the four slots renders: slots 0 and 2 follow TRACK_B, slots 1 and 3 the other size at the same depth, so
    that tiny and large frames are in flight together and every slot's previous frame has the other size"""
    other = {"tiny": "large", "large": "tiny"}
    return [[(name if k % 2 == 0 else other[name], depth) for k in range(TRACK_B_SLOTS)] for name, depth in TRACK_B]


# ---- track C: jitter-table eviction -------------------------------------------------------------------------------------------------
TRACK_C_SLOTS = 3


def K(W, H, spp, band=None, shard=0, n=1):
    """a jitter-table key: the frame's size, its sample count and its shard layout (a full frame: one band of H rows)"""
    return (W, H, spp, H if band is None else band, shard, n)


TRACK_C_KEYS = [K(40, 24, 1), K(40, 24, 2), K(48, 32, 1), K(32, 24, 3), K(40, 24, 2, 8, 0, 2), K(40, 24, 2, 8, 1, 2), K(33, 17, 2),
                K(48, 32, 4, 4, 1, 3), K(16, 16, 5), K(40, 24, 3), K(48, 32, 2, 8, 2, 3)]
# (slot, key index, how): "sync" = rendered and checked at once, "async" = submitted and left pending, "wait" = the pending frame collected
TRACK_C = ([(i % TRACK_C_SLOTS, i, "sync") for i in range(8)] +                       # eight tables: the cache is full
           [(2, 1, "async"),                                                          # slot 2 keeps a frame of key 1 pending ...
            (0, 8, "sync"), (1, 9, "sync"),                                           # ... across two evictions caused by slots 0 and 1
            (2, 1, "wait"),
            (0, 10, "sync"),
            (1, 0, "async"),                                                          # the first key again: its table was evicted and is rebuilt
            (2, 2, "sync"), (0, 3, "sync"),                                           # evicted by now as well: rebuilt while slot 1's frame is pending
            (1, 0, "wait"),
            (2, 0, "sync"), (0, 1, "sync")])


def max_jitter_tables():
    """MAX_JITTER_TABLES of csrc/rt_api.cpp"""
    src = open(os.path.join(ROOT, "vulkan_raytracing_amd", "csrc", "rt_api.cpp")).read()
    m = re.search(r"constexpr\s+size_t\s+MAX_JITTER_TABLES\s*=\s*(\d+)\s*;", src)
    assert m, "MAX_JITTER_TABLES not found in rt_api.cpp"
    return int(m.group(1))


def tail_max_rays():
    """TAIL_MAX_RAYS of csrc/rt_device.h"""
    src = open(os.path.join(ROOT, "vulkan_raytracing_amd", "csrc", "rt_device.h")).read()
    m = re.search(r"constexpr\s+uint32_t\s+TAIL_MAX_RAYS\s*=\s*(\d+)\s*;", src)
    assert m, "TAIL_MAX_RAYS not found in rt_device.h"
    return int(m.group(1))


def simulate_jitter_cache(steps, keys, capacity):
    """the LRU of jitter_table_for over the script: -> [(step index, evicted key index, slots with a frame pending at that moment)]"""
    cache, clock, pending, out = {}, 0, set(), []
    for i, (slot, k, how) in enumerate(steps):
        if how == "wait":
            pending.discard(slot)
            continue
        if k not in cache and len(cache) >= capacity:
            lru = min(cache, key=cache.get)
            del cache[lru]
            out.append((i, lru, sorted(pending)))
        clock += 1
        cache[k] = clock
        if how == "async":
            pending.add(slot)
    return out


# ---- track D: query and shading workspace -------------------------------------------------------------------------------------------
QUERY_SIZES = (5000, 37, 1, 5000)
RAY_HITS_K = (1, 16, 3, 1)       # rt_intersect_device_hits' max_hits along QUERY_SIZES
POINT_HITS_K = (16, 0, 4, 16)    # rt_closest_point_device_hits'
QUERY_KINDS = ("intersect", "intersect_any", "flags", "ray_hits", "closest_point", "point_hits", "overlap_boxes", "overlap_triangles",
               "sweep", "segment", "triangle", "inside", "signed_distance", "shade_library", "shade_caller")
TRACK_D_SEED = 20263
TRACK_D_CHANGES = ("deeper geometry", "first geometry again", "refit_blas_device", "set_instances_device")
SHORT_ROUND_N = 37
CORRIDOR_SQUARES = 4096
