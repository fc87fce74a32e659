"""What rt_refit_blas_device costs, and what it replaces (DESIGN.md §8 "BLAS refit").

Writes one JSON file (default blas_refit_cost_results.json, ignored by git):
  refit        rt_refit_blas_device on the cfg3 stand-in (348 k triangles) and on the teapot, median of --repeats after --warmup calls:
               refit_kernel_ms, the refit alone (HIP events around its kernels on the library's stream, as RT_BUILD_TIMING reports
               them), and refit_call_ms, the host clock around the synchronous call (the wait for frames, the copy, the launches, the
               readback)
  rebuild      the path it replaces: rt_upload_geometry + rt_build_blas of every mesh + rt_set_instances, host clock, median as above
  loop         the animated cfg3 loop with 4 frame slots in flight: rt_set_instances(update) + rt_trace_async per step, without and
               with a refit of the orbiting mesh in every step; the refit waits for the frames of every slot, so that loop
               collects every pending frame before it (the serialisation is part of what it costs)
Usage: python tools/blas_refit_cost.py [--out FILE] [--repeats N] [--warmup N] [--steps N]"""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vulkan_raytracing_amd import RtContext, host, workloads  # noqa: E402

RES = os.path.join(ROOT, "resources")


def deform(verts, idx, ranges, m, phase):
    """mesh m's vertex span displaced along the normals by a sine field (float32 (nv, 6) on the GPU)"""
    import torch
    ff, fi, pc = ranges[m]
    n = 6 * (int(idx[fi:fi + 3 * pc].max()) + 1)
    v = torch.from_numpy(verts[ff:ff + n].reshape(-1, 6).copy()).to("cuda:0")
    p, nrm = v[:, :3], v[:, 3:]
    ext = (p.max(0).values - p.min(0).values).max()
    f = torch.sin(6.0 * p[:, 0] / ext + phase) * torch.sin(7.0 * p[:, 2] / ext)
    return torch.cat([p + 0.05 * ext * f[:, None] * nrm, nrm], dim=1).contiguous()


def median_ms(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def kernel_ms(fn, repeats, warmup):
    """median of the refit's kernel time as the library reports it with RT_BUILD_TIMING (HIP events; stderr captured)"""
    os.environ["RT_BUILD_TIMING"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            for _ in range(warmup + repeats):
                fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["RT_BUILD_TIMING"]
        tmp.seek(0)
        ms = [float(x) for x in re.findall(r"\[blas_refit\].*kernels ([0-9.]+) ms", tmp.read())]
    assert len(ms) == warmup + repeats, ms
    return statistics.median(ms[warmup:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="blas_refit_cost_results.json")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=60)
    a = ap.parse_args()
    import torch
    w = workloads.make("cfg3", RES)
    g = host.SceneGeometry(w.paths)
    res = {"workload": "cfg3", "triangles": [int(r[2]) for r in g.ranges], "repeats": a.repeats, "warmup": a.warmup}
    ctx = RtContext(0)
    ctx.upload_geometry(g.verts, g.idx, g.ranges)
    ctx.set_instances(w.instances)
    ctx.set_uniforms(w.uniforms)
    ctx.set_skybox(w.sky)
    frames = [[deform(g.verts, g.idx, g.ranges, m, 0.1 * k) for k in range(4)] for m in range(len(g.ranges))]
    torch.cuda.synchronize()
    res["refit_kernel_ms"], res["refit_call_ms"] = {}, {}
    for m, name in enumerate(("teapot", "standin")):
        k = [0]

        def one():
            ctx.refit_blas_device(m, frames[m][k[0] % 4])
            k[0] += 1
        res["refit_kernel_ms"][name] = kernel_ms(one, a.repeats, a.warmup)
        res["refit_call_ms"][name] = median_ms(one, a.repeats, a.warmup)
    ctx.set_instances(w.instances)

    def rebuild():
        ctx.upload_geometry(g.verts, g.idx, g.ranges)
        ctx.set_instances(w.instances)
    res["rebuild_ms"] = median_ms(rebuild, a.repeats, a.warmup)

    # the animated loop: 4 slots, the orbiting instance moves every step
    slots = [ctx] + [ctx.frame_slot() for _ in range(3)]
    for s in slots:
        s.set_instances(w.instances)
        s.set_uniforms(w.uniforms)
    anim = host.SceneAnimation()
    loop = {}
    for mode in ("instances_only", "with_refit"):
        pending = [False] * 4
        t0 = None
        for step in range(a.steps + 8):
            if step == 8:
                for i, s in enumerate(slots):
                    if pending[i]:
                        s.trace_wait(copy=False)
                        pending[i] = False
                t0 = time.perf_counter()
            i = step % 4
            if mode == "with_refit":
                for j, s in enumerate(slots):   # (the refit waits for every slot's frame: they are collected first)
                    if pending[j]:
                        s.trace_wait(copy=False)
                        pending[j] = False
                ctx.refit_blas_device(1, frames[1][step % 4])
            elif pending[i]:
                slots[i].trace_wait(copy=False)
                pending[i] = False
            anim.animate(0.01 * step)
            slots[i].set_instances(anim.instances((0, 1)), update=True)
            slots[i].trace_async(w.width, w.height)
            pending[i] = True
        for i, s in enumerate(slots):
            if pending[i]:
                s.trace_wait(copy=False)
        loop[mode] = (time.perf_counter() - t0) * 1e3 / a.steps
    res["loop_ms_per_step"] = loop
    res["frame"] = [w.width, w.height]
    for s in slots[1:]:
        s.close()
    ctx.close()
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
