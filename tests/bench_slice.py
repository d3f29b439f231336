"""The bench-shaped slice that the parity, ladder and paired-launch tests and three diagnostic tools share (test infrastructure, no tests in here): a ~100 k-voxel
cap of the bench scene family (1 mm voxels, thin-shell factor 1, bumpy sphere), ALL 200 keyframes at 640x480 with the bench's pose / luminance noise, spatially
varying SH; the shipped lambda schedule; the state its second outer iteration starts from; the runs of the single-rank and the simulated sharded solver on it.

`slice_setup` is a module-scoped fixture: a test module takes it by name (`from bench_slice import slice_setup  # noqa: F401`) and gets its own slice.

The asserts in here are not rewritten by pytest: each carries its own message."""
import numpy as np
import pytest

import helpers


def build_slice(O):
    from intrinsic3d_amd import synthetic
    rv = 72
    sc = synthetic.make_scene(radius_vox=rv, voxel_size=0.001, K=200, width=640, height=480, levels=1, band_vox=3.5, seed=1234,
                              cam_dist=2.6 * rv * 0.001, pose_noise=(0.002, 0.0035), lum_noise=0.005, bump_amp_vox=0.5, bump_freq=40.0)
    keys = sc["keys"]; x = keys[:, 0]
    n_target = 100_000
    cut = np.partition(x, len(x) - n_target)[len(x) - n_target]
    sel = x >= cut
    thres = 1.0 * float(sc["voxel_size"])
    g = O.Grid.from_voxels(sc["voxel_size"], keys[sel], sc["sdf"][sel], sc["weight"][sel], sc["color"][sel])
    fr = O.Frames(sc["frames"], 1)
    rc, sh, idx, vsh, has, st = O.estimate_sh(g, 0.03, 10.0, thres)
    assert rc == 0 and sh.shape[0] >= 8, (rc, sh.shape)          # several SH subvolumes, as in the bench
    arrays = g.export()
    return dict(O=O, sc=sc, g=g, fr=fr, arrays=arrays, vsh=vsh, thres=thres)


@pytest.fixture(scope="module")
def slice_setup(oracle):
    return build_slice(oracle)


def bench_cfg(O, thres, cg_fixed, second=False):
    # the shipped schedule over 2 outer iterations (cost.h:130-143): iteration 0 uses (lambda_r0, lambda_s0), iteration 1 (lambda_r1, lambda_s1).
    # Each iteration is run as its own call from IDENTICAL inputs on both sides (see run_both), so the second call carries the end values.
    lr, ls = (10.0, 10.0) if second else (80.0, 120.0)
    return helpers.oracle_cfg(O, thres, iterations=1, lm_steps=50, lambda_g=0.2, lambda_r0=lr, lambda_r1=lr, lambda_s0=ls, lambda_s1=ls,
                              lambda_a=0.1, fix_poses=0, fix_intrinsics=0, fix_distortion=0, occlusion_distance=0.02, num_observations=5,
                              cg_fixed_iterations=cg_fixed)


def run_both(S, cg_fixed):
    """Two outer iterations, each from bit-identical inputs on both sides: the device's second iteration starts from the ORACLE's state after
    the first.  (Chaining the device's own first result instead makes the comparison flip between two outcomes from run to run: the fp32
    atomics leave the first result reproducible to 1e-7 only, which is enough to swap two keyframes of near-equal weight at the top-5 cut
    of one voxel (colorization.cpp:357-370) and with it one Eg row — a discrete decision of the reference algorithm, not a solver error.
    Measured: 4e-4 on the albedo around voxel (123, 82, 142) of this scene in about half of the runs, also with the round-1 kernels.)"""
    O = S["O"]; sc = S["sc"]; a0 = S["arrays"]
    S["g"].import_fields(sdf_refined=a0["sdf_refined"], albedo=a0["albedo"], color=a0["color"])      # the oracle run mutates its grid
    out = []
    arrays = a0; cam = (sc["intr"], sc["dist"], sc["poses"])
    for second in (False, True):
        ocfg = bench_cfg(O, S["thres"], cg_fixed, second)
        sc_it = dict(sc); sc_it["intr"], sc_it["dist"], sc_it["poses"] = cam
        ctx = helpers.gpu_context(sc_it, arrays, S["vsh"])
        gst = ctx.optimize(helpers.gpu_cfg(ocfg))
        sdf, alb = ctx.get_grid(); gi, gd, gp = ctx.get_camera()
        ctx.close()
        rc, intr, dist, poses, ostats = O.optimize(S["g"], S["fr"], ocfg, cam[0], cam[1], cam[2], S["vsh"])
        assert rc == 0, ("oracle optimize", rc)
        ref = S["g"].export()
        out.append((ref, (intr, dist, poses), ostats[0], (sdf, alb), (gi, gd, gp), gst[0], arrays))
        arrays = ref; cam = (intr, dist, poses)
    return out


def run(S, iterations=2, cg_fixed=-1):
    """(stats, sdf, albedo, camera, ladder stats) of chained outer iterations from the slice's start, single rank"""
    O = S["O"]; sc = S["sc"]; a0 = S["arrays"]
    cfg = helpers.gpu_cfg(bench_cfg(O, S["thres"], cg_fixed)); cfg.iterations = iterations
    ctx = helpers.gpu_context(sc, a0, S["vsh"])
    st = ctx.optimize(cfg); sdf, alb = ctx.get_grid(); cam = ctx.get_camera(); lad = ctx.debug_ladder_stats(); ctx.close()
    return st, sdf, alb, cam, lad


def stats(st):
    return [(s.num_attempts, list(s.step_accepted[:s.num_attempts]), list(s.pcg_iterations[:s.num_attempts]), s.cost_initial, s.cost_final, s.final_radius, s.termination,
             list(s.rows)) for s in st]


_second = {}


def second_iteration_start(S):
    """The state the SECOND outer iteration of the bench slice starts from (the first one, one accepted attempt, run once on a single rank in the bit-reproducible default
    mode): the iteration with the rejected attempts — the one the ladder is about — then starts from IDENTICAL inputs in every variant compared with it.  (Chaining the two
    iterations inside every variant instead makes the comparison bistable: the variants' first results differ by round-off, which is enough to swap two keyframes of
    near-equal weight at the top-5 cut of one voxel, colorization.cpp:357-370 — a discrete decision of the reference algorithm — and the fields around it then end 5.3e-4
    apart in about half of the runs, sharded or not: tools/experiments/sharded_ladder_diag.py, and run_both for the same voxel in round 1.)
    Computed once per process: host arrays only, no device handle is kept."""
    if "start" not in _second:
        O = S["O"]; sc = S["sc"]
        cfg = helpers.gpu_cfg(bench_cfg(O, S["thres"], -1, second=False))
        ctx = helpers.gpu_context(sc, S["arrays"], S["vsh"])
        st = ctx.optimize(cfg); sdf, alb = ctx.get_grid(); cam = ctx.get_camera(); ctx.close()
        assert st[0].successful_steps == 1, ("successful steps of the first iteration", st[0].successful_steps)
        arrays = dict(S["arrays"]); arrays["sdf_refined"] = sdf; arrays["albedo"] = alb
        sc2 = dict(sc); sc2["intr"], sc2["dist"], sc2["poses"] = cam
        _second["start"] = (sc2, arrays)
    return _second["start"]


def run_ranks(S, W, cg_fixed=-1):
    """W simulated ranks (host threads on one GPU, i3d_comm_init_sim) through the second outer iteration of the bench slice: per rank (stats, sdf, albedo, camera, ladder stats, comm stats)"""
    import threading
    from intrinsic3d_amd import binding
    sc2, arrays = second_iteration_start(S)
    cfg = helpers.gpu_cfg(bench_cfg(S["O"], S["thres"], cg_fixed, second=True))
    L = binding.load()
    shared = L.i3d_comm_sim_create(W)
    ctxs = [helpers.gpu_context(sc2, arrays, S["vsh"]) for _ in range(W)]
    for r, c in enumerate(ctxs):
        c.comm_init_sim(shared, r)
    out = [None] * W; err = [None] * W

    def work(r):
        try:
            out[r] = ctxs[r].optimize(cfg)
        except Exception as e:      # surface failures instead of deadlocking the other ranks silently
            err[r] = e
    th = [threading.Thread(target=work, args=(r,)) for r in range(W)]
    [t.start() for t in th]; [t.join(timeout=300) for t in th]
    assert not any(t.is_alive() for t in th), "sharded run hung"
    assert all(e is None for e in err), err
    res = []
    for r, c in enumerate(ctxs):
        sdf, alb = c.get_grid(); res.append((out[r], sdf, alb, c.get_camera(), c.debug_ladder_stats(), c.comm_stats())); c.close()
    L.i3d_comm_sim_destroy(shared)
    return res


def color_frames(sc):
    """give the keyframes three different colour channels (the synthetic renderer emits grey)"""
    frames = []
    for fr in sc["frames"]:
        bgrs = []
        for b in fr["bgr"]:
            g = b[..., 0].astype(np.float32)
            bgrs.append(np.stack([0.7 * g, g, 255.0 - 0.5 * g], axis=-1).astype(np.uint8))
        frames.append({"lum": fr["lum"], "depth": fr["depth"], "bgr": bgrs})
    return frames
