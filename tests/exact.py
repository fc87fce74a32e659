"""Exact comparison of GPU results with the oracle (frames and hit records equal the oracle's bit for bit).

There is no tolerance.  Pixels are compared as bits (RGBA32F frames through their uint32 words, 8-bit frames byte for byte), so
+0.0 against -0.0 and NaN against NaN are differences.  On a mismatch the message says which side is wrong: up to 64 of the differing
pixels (rays) are resolved again with the oracle's brute-force mode, which walks no tree, and the message reports whether the GPU or
the oracle's BVH mode agrees with it.  The oracle scene passed in must still be in the state that rendered the reference."""
import numpy as np

SHOW = 20        # differing pixels / rays listed in a failure message
ARBITRATE = 64   # differing pixels / rays re-resolved by brute force


def _bits(img):
    img = np.ascontiguousarray(img)
    if img.dtype == np.float32:
        return img.view(np.uint32)
    if img.dtype == np.uint8:
        return img
    raise TypeError("frames are RGBA32F or 8-bit, not %s" % img.dtype)


def quantize8(img, bgra=False):
    """the 8-bit frame of a RGBA32F frame as the kernels store it (rt_set_param "output_rgba8" / "output_bgra8"): clamp, x255, round"""
    q = (np.clip(img, 0.0, 1.0) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
    return q[..., [2, 1, 0, 3]] if bgra else q


def _as_gpu_format(px, gpu_dtype, bgra):
    return quantize8(px, bgra) if gpu_dtype == np.uint8 else np.asarray(px, np.float32)


def _same(a, b):
    return bool(np.array_equal(_bits(a), _bits(b)))


def frame_mismatch(gpu, ref, y0=0, y1=None):
    """(x, y) of every pixel of rows [y0, y1) whose bits differ in any channel, in row-major order"""
    gpu, ref = np.asarray(gpu), np.asarray(ref)
    assert gpu.shape == ref.shape and gpu.dtype == ref.dtype, (gpu.shape, gpu.dtype, ref.shape, ref.dtype)
    y1 = gpu.shape[0] if y1 is None else y1
    d = (_bits(gpu[y0:y1]) != _bits(ref[y0:y1])).any(axis=2)
    ys, xs = np.nonzero(d)
    return np.stack([xs, ys + y0], axis=1).astype(np.uint32)


def assert_frame_equals_oracle(gpu, orc, W, H, y0=0, y1=None, ref=None, bgra=False):
    """Rows [y0, y1) of the H x W frame `gpu` (RGBA32F, or 8-bit RGBA / BGRA with bgra=True) equal the oracle's frame bit for bit.

    ref: the oracle's RGBA32F frame (H rows; only rows [y0, y1) are read), rendered here with orc.render when None.  orc: the oracle
    scene that rendered ref, in that state still (it re-renders differing pixels by brute force).  Returns the RGBA32F oracle frame."""
    y1 = H if y1 is None else y1
    gpu = np.asarray(gpu)
    assert gpu.shape == (H, W, 4), (gpu.shape, H, W)
    if ref is None:
        ref, _ = orc.render(W, H, y0=y0, y1=y1)
    ref = np.asarray(ref, np.float32)
    want = _as_gpu_format(ref, gpu.dtype, bgra)
    bad = frame_mismatch(gpu, want, y0, y1)
    if len(bad) == 0:
        return ref
    msg = ["%d of %d pixels of rows %d..%d differ from the oracle (bits)" % (len(bad), W * (y1 - y0), y0, y1 - 1)]
    g = gpu[bad[:, 1], bad[:, 0]]
    o = want[bad[:, 1], bad[:, 0]]
    with np.errstate(invalid="ignore"):
        ad = np.abs(g.astype(np.float64) - o.astype(np.float64))
    msg.append("largest absolute difference %r%s" % (float(np.nanmax(ad)) if not np.isnan(ad).all() else float("nan"),
                                                     " (and NaN on one side)" if np.isnan(ad).any() else ""))
    for k in range(min(SHOW, len(bad))):
        msg.append("  (x %d, y %d) gpu %s oracle %s" % (bad[k, 0], bad[k, 1], g[k].tolist(), o[k].tolist()))
    xy = bad[:ARBITRATE]
    bf = _as_gpu_format(orc.render_pixels(W, H, xy, use_bvh=False), gpu.dtype, bgra)
    gpu_ok = [_same(g[k], bf[k]) for k in range(len(xy))]
    orc_ok = [_same(o[k], bf[k]) for k in range(len(xy))]
    msg.append("brute force re-render of %d of them: the GPU agrees on %d, the oracle's BVH mode on %d, neither on %d"
               % (len(xy), sum(gpu_ok), sum(orc_ok), sum(1 for a, b in zip(gpu_ok, orc_ok) if not a and not b)))
    for k in range(min(SHOW, len(xy))):
        side = "GPU" if gpu_ok[k] else ("oracle BVH" if orc_ok[k] else "neither")
        msg.append("  (x %d, y %d) brute force %s: sides with %s" % (xy[k, 0], xy[k, 1], bf[k].tolist(), side))
    raise AssertionError("\n".join(msg))


def _hit_words(h):
    h = np.ascontiguousarray(h)
    return np.stack([h["t"].view(np.uint32), h["u"].view(np.uint32), h["v"].view(np.uint32),
                     h["prim"].view(np.uint32), h["inst"].view(np.uint32)], axis=1)


def hit_mismatch(a, b):
    """indices of the records whose fields (t, u, v, prim, inst) differ in any bit"""
    assert len(a) == len(b)
    return np.nonzero((_hit_words(a) != _hit_words(b)).any(axis=1))[0]


def assert_hits_equal_oracle(gpu, orc, rays, any_hit=False, ref=None):
    """Every hit record of the GPU equals the oracle's BVH mode in every field, bit for bit.  The differing rays are resolved again
    by brute force (orc.intersect(use_bvh=False)) and the message says which side it agrees with.  Returns the oracle's records."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    if ref is None:
        ref = orc.intersect(rays, any_hit=any_hit, use_bvh=True)
    bad = hit_mismatch(gpu, ref)
    if len(bad) == 0:
        return ref
    bf = orc.intersect(rays[bad[:ARBITRATE]], any_hit=any_hit, use_bvh=False)
    sub_g, sub_o = np.asarray(gpu)[bad[:ARBITRATE]], np.asarray(ref)[bad[:ARBITRATE]]
    gpu_ok = _hit_words(sub_g) == _hit_words(bf)
    orc_ok = _hit_words(sub_o) == _hit_words(bf)
    gpu_ok, orc_ok = gpu_ok.all(axis=1), orc_ok.all(axis=1)
    msg = ["%d of %d hit records differ from the oracle's BVH mode (bits)" % (len(bad), len(rays)),
           "brute force on %d of them: the GPU agrees on %d, the oracle's BVH mode on %d, neither on %d"
           % (len(sub_g), int(gpu_ok.sum()), int(orc_ok.sum()), int((~gpu_ok & ~orc_ok).sum()))]
    for k in range(min(SHOW, len(sub_g))):
        side = "GPU" if gpu_ok[k] else ("oracle BVH" if orc_ok[k] else "neither")
        msg.append("  ray %d: gpu %s oracle %s brute force %s: sides with %s" % (bad[k], sub_g[k], sub_o[k], bf[k], side))
    raise AssertionError("\n".join(msg))

