"""Replay of the records that tests/golden/make_spirv_fixtures.py made by interpreting the reference's compiled shaders, shared by
the base set (tests/test_oracle.py) and the edge set (tests/test_spirv_edge.py).

Bars: 1e-5 absolute (GLSL leaves the precision of normalize / reflect / pow / dot open, so bit equality with any one implementation
is not defined), 2e-5 on the lit colour because pow(x, 100) by repeated squaring carries up to ~100 half-ulps of a term <= 0.8."""
import numpy as np

SPV_TOL, SPV_TOL_LIT = 1e-5, 2e-5
AMBIENT = np.array([0.08, 0.24, 0.08], np.float32)      # Iamb * ka


def replay_records(fixture_scenes, oracle_scene=None):
    """rgen prologue (jitter hash, primary ray), rchit (closest_hit_attributes) and one bounce-loop iteration (bounce_step) of every
    record against what the reference's shader.rgen.spv / shader.rchit.spv / miss modules computed for the same inputs.  Control flow
    and integers are asserted here; returns the worst absolute difference per quantity, for the caller to hold to SPV_TOL.
    oracle_scene(sc) -> the oracle scene of a fixture scene (default: sc.oracle_scene())."""
    from oracle.oracle import HIT_DTYPE
    worst = {}

    def track(key, err):
        worst[key] = max(worst.get(key, 0.0), float(err))

    for sc in fixture_scenes:
        S, b, W, H = (oracle_scene(sc) if oracle_scene else sc.oracle_scene()), sc.bounces, sc.width, sc.height
        # -- src/shader.rgen:57-79: the primary ray of every sample
        f = b[b["bounce"] == 0]
        od = np.array([S.primary_ray(int(r["px"]), int(r["py"]), W, H, int(r["sample"])) for r in f])
        assert np.array_equal(od[:, 0:3], f["o"])
        track("primary ray", np.abs(od[:, 3:6] - f["d"]).max())
        # -- the traversal the fixture was made with is this scene's (meshes regenerate identically, instances decode)
        rays = np.zeros((len(b), 8), np.float32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = b["o"], 0.001, b["d"], 10000.0
        h = S.intersect(rays)
        for k in ("prim", "inst"):
            assert np.array_equal(h[k], b[k]), sc.name
        assert np.array_equal(h["t"].view(np.uint32), b["t"].view(np.uint32))
        # -- one loop iteration per record
        hits = np.zeros(len(b), HIT_DTYPE)
        for k in ("t", "u", "v", "prim", "inst"):
            hits[k] = b[k]
        st = S.bounce_step(np.concatenate([b["o"], b["d"]], axis=1), b["sample"].astype(np.uint32), hits)
        kind = st[:, 0].astype(int)
        hit, miss = b["inst"] >= 0, b["inst"] < 0
        # rmiss: objectIndex = -1, sky colour, loop ends           (src/shader.rmiss:11, src/shader.rgen:90-94)
        assert np.all(kind[miss] == 0) and np.all(b["object_index"][miss] == -1) and np.all(b["last"][miss] == 1)
        if miss.any():
            track("sky colour", np.abs(st[miss, 24:27] - b["color"][miss]).max())
        # rchit payload                                             (src/shader.rchit:50-96)
        assert np.array_equal(st[hit, 7].astype(int), b["object_index"][hit])
        track("payload.hitPosition", np.abs(st[hit, 1:4] - b["P"][hit]).max())
        track("payload.hitNormal", np.abs(st[hit, 4:7] - b["N"][hit]).max())
        # diffuse: back-face break, or shadow ray + Blinn-Phong      (src/shader.rgen:97-131)
        sh = b["shadow"] == 1
        assert np.array_equal(kind == 2, sh), sc.name
        if sh.any():
            track("shadow ray origin", np.abs(st[sh, 8:11] - b["so"][sh]).max())
            track("shadow ray direction", np.abs(st[sh, 11:14] - b["sl"][sh]).max())
            track("shadow ray tmax", np.abs(st[sh, 14] - b["stmax"][sh]).max())
            lit = sh & (b["occluded"] == 0)
            if lit.any():
                track("lit colour", np.abs(st[lit, 15:18] - b["color"][lit]).max())
            dark = sh & (b["occluded"] == 1)
            assert np.all(b["color"][dark] == AMBIENT)            # tmpColor keeps Iamb*ka
        back = kind == 1
        assert np.all(b["last"][back] == 1) and np.all(b["color"][back] == AMBIENT)
        # mirror / refract / TIR: the next ray                       (src/shader.rgen:132-165)
        cont = kind == 3
        go_on = cont & (b["last"] == 0)
        assert np.array_equal(b["last"] == 0, go_on)                # the recorded loop continued exactly where bounce_step says so
        if go_on.any():
            track("next rayOrigin", np.abs(st[go_on, 18:21] - b["no"][go_on]).max())
            track("next rayDirection", np.abs(st[go_on, 21:24] - b["nd"][go_on]).max())
        ended = cont & (b["last"] == 1)                             # bounce budget exhausted: j == maxBounceCount
        assert np.all(b["bounce"][ended] == int(sc.uniforms[0]["max_bounce_count"]))
    return worst
