"""The colour of caller-generated primary rays (rt_shade_rays_device), composed from the oracle's exports: for every live ray the bounce
loop of src/shader.rgen:84-177 runs as orc.intersect (closest hit; the first segment over [0.001, tmax of the record], the later ones
over [0.001, 10000]), orc.bounce_step, and on STEP_SHADOW an any-hit orc.intersect of the shadow ray.  Nothing here restates the
shading arithmetic: it is the oracle's own bounce step, the same code orc.render runs."""
import numpy as np

STEP_SKY, STEP_BACKFACE, STEP_SHADOW, STEP_CONTINUE = 0, 1, 2, 3
# Iamb * ka as glslang folded it into shaders/shader.rgen.spv (the oracle's kAmbient)
AMBIENT = np.array([0x3DA3D70A, 0x3E75C28F, 0x3DA3D70A], np.uint32).view(np.float32)


def valid_records(rays):
    """records that are rays: finite origin and direction, direction not zero"""
    o, d = rays[:, 0:3], rays[:, 4:7]
    return np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)


def shade_samples(orc, rays, n_points, max_bounce, instances=None, ranges=None, materials=None):
    """(n, 4) float32 per-sample colours of the n = len(rays) records (sample-major: record i * n_points + p is sample i of point p).
    With a material table (materials = (table, prim_material)), `instances` and `ranges` locate the hit triangle's material, whose
    Iamb * ka = float32(0.8) * ka is the colour of an occluded shadow ray (orc_bounce_step's 28 floats do not carry it)."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    n = len(rays)
    out = np.zeros((n, 4), np.float32)
    live = np.nonzero(valid_records(rays))[0]
    out[live, 0:3] = AMBIENT   # what the loop leaves when the bounce budget ends (and STEP_BACKFACE)
    out[live, 3] = 1.0
    sample_index = (np.arange(n, dtype=np.int64) // max(n_points, 1)).astype(np.uint32)
    idx = live
    o, d = rays[live, 0:3].copy(), rays[live, 4:7].copy()
    tmax = rays[live, 7].copy()
    for j in range(int(max_bounce) + 1):
        if len(idx) == 0:
            break
        r8 = np.zeros((len(idx), 8), np.float32)
        r8[:, 0:3] = o; r8[:, 3] = 0.001; r8[:, 4:7] = d
        r8[:, 7] = tmax if j == 0 else 10000.0
        hits = orc.intersect(r8)
        st = orc.bounce_step(np.concatenate([o, d], 1), sample_index[idx], hits)
        kind = st[:, 0].astype(np.int32)
        sky = kind == STEP_SKY
        out[idx[sky], 0:3] = st[sky, 24:27]
        sh = np.nonzero(kind == STEP_SHADOW)[0]
        if len(sh):
            s8 = np.zeros((len(sh), 8), np.float32)
            s8[:, 0:3] = st[sh, 8:11]; s8[:, 3] = 0.001; s8[:, 4:7] = st[sh, 11:14]; s8[:, 7] = st[sh, 14]
            occ = orc.intersect(s8, any_hit=True)["inst"] >= 0
            col = st[sh, 15:18].copy()
            amb = np.broadcast_to(AMBIENT, (len(sh), 3)).copy()
            if materials is not None:
                table, prim_material = materials
                h = hits[sh]
                first = np.array([ranges[int(instances[i]["mesh"])][1] // 3 for i in h["inst"]], np.int64)
                mat = np.asarray(prim_material)[first + h["prim"]]
                amb = np.float32(0.8) * np.asarray(table["ka"], np.float32)[mat]
            col[occ] = amb[occ]
            out[idx[sh], 0:3] = col
        cont = kind == STEP_CONTINUE
        idx = idx[cont]
        o, d = st[cont, 18:21].copy(), st[cont, 21:24].copy()
    return out


def average_points(samples, n_points, n_samples):
    """the frame's resolve (src/shader.rgen:178-183): ordered float32 sum over the samples of a point, then one division"""
    acc = np.zeros((n_points, 4), np.float32)
    for i in range(n_samples):
        acc = acc + samples[i * n_points:(i + 1) * n_points]
    return acc / np.float32(n_samples)


def pinhole_rays(orc, W, H, spp, tmax=10000.0):
    """the primary rays of a W x H frame at spp samples (orc.primary_ray: src/shader.rgen:62-82) as rt_shade_rays_device records,
    sample-major like the frame's sample ids: record i * W * H + y * W + x"""
    rays = np.zeros((spp * H * W, 8), np.float32)
    k = 0
    for i in range(spp):
        for y in range(H):
            for x in range(W):
                od = orc.primary_ray(x, y, W, H, i)
                rays[k, 0:3] = od[0:3]; rays[k, 4:7] = od[3:6]
                k += 1
    rays[:, 7] = tmax
    return rays
