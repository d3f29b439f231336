"""-m gpu: oracle parity at the PCG depth bench.py actually runs.

A bench-shaped slice: a ~100 k-voxel cap of the bench scene family (1 mm voxels, thin-shell factor 1, bumpy sphere), ALL 200 keyframes at
640x480 with the bench's pose / luminance noise, spatially varying SH, every parameter group free, the shipped lambda schedule.  Two outer
iterations against the fp64 oracle (nls_solver.cpp:296-337 semantics) with
  (a) 30 PCG iterations per LM attempt (three residual resets, deeper than any attempt of the bench), and
  (b) Ceres' own quadratic-model stopping rule (pcg_fixed_iterations = -1), the mode bench.py times.
Asserted: row counts, accept / reject sequence of every LM attempt, PCG iteration counts (native; +-1 tolerated only where stated), and
sdf / albedo / poses / intrinsics at the north-star 1e-4."""
import numpy as np
import pytest

import helpers
from bench_slice import bench_cfg, run_both
from bench_slice import slice_setup  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def _check_fields(ref, ocam, dev, dcam, start):
    sdf, alb = dev; intr, dist, poses = ocam; gi, gd, gp = dcam
    e_sdf = np.abs(sdf - ref["sdf_refined"]).max() / np.abs(ref["sdf_refined"]).max()
    e_alb = np.abs(alb - ref["albedo"]).max() / np.abs(ref["albedo"]).max()
    assert e_sdf <= 1e-4, e_sdf
    assert e_alb <= 1e-4, e_alb
    # the STEP itself (not just the state it is added to) is reproduced: error relative to the largest update of the iteration
    u_sdf = np.abs(ref["sdf_refined"] - start["sdf_refined"]).max(); u_alb = np.abs(ref["albedo"] - start["albedo"]).max()
    assert np.abs(sdf - ref["sdf_refined"]).max() <= 1e-3 * u_sdf and np.abs(alb - ref["albedo"]).max() <= 1e-3 * u_alb
    np.testing.assert_allclose(gi, intr, rtol=1e-4)
    np.testing.assert_allclose(gp, poses, rtol=1e-4, atol=1e-6)
    return e_sdf, e_alb


def test_deep_fixed_pcg_matches_oracle(slice_setup):
    """30 PCG iterations per attempt: r = b - A x is re-formed at iterations 10, 20, 30 (residual_reset_period)."""
    runs = run_both(slice_setup, 30)
    for ref, ocam, so, dev, dcam, sg, start in runs:
        assert list(so.rows) == list(sg.rows) and so.rows[0] > 100_000
        assert so.n_attempts == sg.num_attempts
        assert list(so.accepted[:so.n_attempts]) == list(sg.step_accepted[:sg.num_attempts])
        assert list(so.cg_iters[:so.n_attempts]) == list(sg.pcg_iterations[:sg.num_attempts]) == [30] * so.n_attempts
        assert abs(so.cost_initial - sg.cost_initial) <= 1e-4 * so.cost_initial and abs(so.cost_final - sg.cost_final) <= 1e-4 * so.cost_final
        _check_fields(ref, ocam, dev, dcam, start)
    assert sum(r[2].n_attempts for r in runs) >= 4             # rejected attempts (radius re-discovery, optimizer.cpp:138) are part of the comparison


def test_untiled_fallback_at_bench_depth(slice_setup, monkeypatch):
    """The round-1 operator (k_eg_jtjp + k_gather, six launches per pass) is what a single rank falls back to when a tile's halo does not fit; it stays in
    the library for that case only, so it gets the same bar as the tiled pass: 30 PCG iterations per attempt against the fp64 oracle."""
    monkeypatch.setenv("I3D_NO_TILE", "1")
    runs = run_both(slice_setup, 30)
    for ref, ocam, so, dev, dcam, sg, start in runs:
        assert list(so.rows) == list(sg.rows)
        assert list(so.accepted[:so.n_attempts]) == list(sg.step_accepted[:sg.num_attempts])
        assert list(so.cg_iters[:so.n_attempts]) == list(sg.pcg_iterations[:sg.num_attempts]) == [30] * so.n_attempts
        _check_fields(ref, ocam, dev, dcam, start)


def test_native_pcg_stop_matches_oracle(slice_setup, monkeypatch):
    """Ceres' quadratic-model stop (eta = 0.1) decided on the device from fp32 vectors / fp64 reductions vs the fp64 oracle: the
    iteration count of every LM attempt, the accept / reject sequence and the accepted step.  In the LDS-ATOMIC mode (I3D_DETERMINISTIC=0: the default of
    rounds 1-4 and of a sharded run's lone-system passes), whose run-to-run summation-order noise is what the +-1 on rejected attempts below covers; the test
    behind this one holds the bit-reproducible mode (the default on one rank) to the exact counts."""
    monkeypatch.setenv("I3D_DETERMINISTIC", "0")
    for ref, ocam, so, dev, dcam, sg, start in run_both(slice_setup, -1):
        assert list(so.rows) == list(sg.rows)
        assert so.n_attempts == sg.num_attempts
        assert list(so.accepted[:so.n_attempts]) == list(sg.step_accepted[:sg.num_attempts])
        oc = list(so.cg_iters[:so.n_attempts]); gc = list(sg.pcg_iterations[:sg.num_attempts])
        # the stop test compares i*(Q1-Q0)/Q1 with 0.1: fp32 vector round-off may move a REJECTED attempt's count by one;
        # the attempt whose step is accepted must stop at the same iteration
        assert all(abs(a - b) <= 1 for a, b in zip(oc, gc)), (oc, gc)
        assert oc[-1] == gc[-1], (oc, gc)
        assert abs(so.cost_final - sg.cost_final) <= 1e-4 * so.cost_final
        _check_fields(ref, ocam, dev, dcam, start)


def test_native_pcg_stop_in_the_bit_reproducible_mode(slice_setup, monkeypatch):
    """The same comparison with every device sum in a fixed order (I3D_DETERMINISTIC=1): no tolerance on the PCG iteration counts — every attempt, rejected or accepted,
    stops at the iteration the fp64 oracle stops at on this slice (the +-1 of the test above covers run-to-run summation-order noise of the default mode, which this
    mode does not have)."""
    monkeypatch.setenv("I3D_DETERMINISTIC", "1")
    for ref, ocam, so, dev, dcam, sg, start in run_both(slice_setup, -1):
        assert list(so.rows) == list(sg.rows) and so.n_attempts == sg.num_attempts
        assert list(so.accepted[:so.n_attempts]) == list(sg.step_accepted[:sg.num_attempts])
        assert list(so.cg_iters[:so.n_attempts]) == list(sg.pcg_iterations[:sg.num_attempts]), (list(so.cg_iters[:so.n_attempts]), list(sg.pcg_iterations[:sg.num_attempts]))
        _check_fields(ref, ocam, dev, dcam, start)


def test_chained_ten_iterations_without_reseeding(slice_setup):
    """Ten CHAINED outer iterations (the shipped lambda schedule, Ceres' own PCG stop, every group free) on the bench-shaped slice: the device continues
    from ITS OWN result and the oracle from its own — no re-seeding.  The two states differ by fp32 round-off, which a handful of discrete decisions of
    the reference algorithm amplify: where two keyframes sit within round-off of each other at the top-5 cut (colorization.cpp:357-370), or a projection
    lands within round-off of a pixel boundary (camera.cpp:148-151), the two sides give a voxel a different Eg row.  The test therefore
      * tracks, iteration by iteration, the voxels whose (voxel, keyframe) row sets differ, and holds their number to a small bound;
      * shows that such flips are near-ties: the oracle's top-5 margin (orc_observation_margins) of most of them is tiny;
      * holds EVERYTHING farther than 2 voxels from a flipped voxel to the north-star 1e-4, and the camera too."""
    import json, os
    S = slice_setup; O = S["O"]; sc = S["sc"]; a0 = S["arrays"]; N = len(a0["keys"]); iters = 10
    S["g"].import_fields(sdf_refined=a0["sdf_refined"], albedo=a0["albedo"], color=a0["color"])
    ctx = helpers.gpu_context(sc, a0, S["vsh"])
    cam = (sc["intr"], sc["dist"], sc["poses"])
    flipped = np.zeros(N, bool); log = []
    for it in range(iters):
        lr = 80.0 + (10.0 - 80.0) / (iters - 1) * it; ls = 120.0 + (10.0 - 120.0) / (iters - 1) * it          # computeVaryingLambda, cost.h:130-143
        ocfg = helpers.oracle_cfg(O, S["thres"], iterations=1, lm_steps=50, lambda_g=0.2, lambda_r0=lr, lambda_r1=lr, lambda_s0=ls, lambda_s1=ls, lambda_a=0.1,
                                  occlusion_distance=0.02, num_observations=5, cg_fixed_iterations=-1)
        gcfg = helpers.gpu_cfg(ocfg)
        # the rows each side assembles at its own state
        pv = O.ProblemView(S["g"], S["fr"], ocfg, cam[0], cam[1], cam[2], S["vsh"]); vo, fo, _, _, _ = pv.eg(with_jacobian=False); pv.free()
        ctx.debug_assemble(gcfg, 0); gfr = ctx.debug_eg_rows(jac=False)[0]
        K = sc["K"]
        om = np.zeros((N, K), bool); om[vo, fo] = True
        gm = np.zeros((N, K), bool); vv, ss = np.nonzero(gfr >= 0); gm[vv, gfr[vv, ss]] = True
        diff = (om != gm).any(axis=1)
        margins = O.observation_margins(S["g"], S["fr"], ocfg, cam[0], cam[1], cam[2])
        log.append({"iteration": it, "rows_oracle": int(om.sum()), "rows_device": int(gm.sum()), "voxels_with_other_rows": int(diff.sum()),
                    "of_them_margin_below_1e-3": int((diff & (margins >= 0) & (margins < 1e-3)).sum()), "margin_below_1e-5_all": int(((margins >= 0) & (margins < 1e-5)).sum())})
        flipped |= diff
        gst = ctx.optimize(gcfg)
        rc, intr, dist, poses, ost = O.optimize(S["g"], S["fr"], ocfg, cam[0], cam[1], cam[2], S["vsh"]); assert rc == 0
        cam = (intr, dist, poses)
        log[-1].update(attempts=[int(ost[0].n_attempts), int(gst[0].num_attempts)], cost_final=[ost[0].cost_final, gst[0].cost_final])
    ref = S["g"].export(); sdf, alb = ctx.get_grid(); gi, gd, gp = ctx.get_camera(); ctx.close()
    # voxels within 2 cells of a flipped voxel are excluded (a different Eg row moves its 14-voxel stencil and, through the regularisers, its ring)
    keys = a0["keys"]; kmin = keys.min(0) - 3; dims = keys.max(0) - kmin + 4
    vol = np.zeros(dims, bool); fk = keys[flipped] - kmin
    for dx in range(-2, 3):
        for dy in range(-2, 3):
            for dz in range(-2, 3):
                vol[fk[:, 0] + dx, fk[:, 1] + dy, fk[:, 2] + dz] = True
    kk = keys - kmin; excluded = vol[kk[:, 0], kk[:, 1], kk[:, 2]]
    e_sdf = np.abs(sdf - ref["sdf_refined"]) / np.abs(ref["sdf_refined"]).max(); e_alb = np.abs(alb - ref["albedo"]) / np.abs(ref["albedo"]).max()
    summary = {"voxels": N, "flipped_voxels": int(flipped.sum()), "excluded_voxels": int(excluded.sum()), "max_err_sdf_kept": float(e_sdf[~excluded].max()),
               "max_err_albedo_kept": float(e_alb[~excluded].max()), "max_err_sdf_all": float(e_sdf.max()), "max_err_albedo_all": float(e_alb.max()),
               "q999_sdf_all": float(np.quantile(e_sdf, 0.999)), "q999_albedo_all": float(np.quantile(e_alb, 0.999)),
               "intr_rel": float(np.abs((gi - cam[0]) / cam[0]).max()), "poses_abs": float(np.abs(gp - cam[2]).max()), "per_iteration": log}
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "chained_parity.json"), "w") as f:
            json.dump(summary, f, indent=1)
    assert summary["flipped_voxels"] <= 0.01 * N, summary                                   # a handful per iteration, none of them a solver difference
    assert summary["excluded_voxels"] <= 0.25 * N, summary
    assert summary["max_err_sdf_kept"] <= 1e-4 and summary["max_err_albedo_kept"] <= 1e-4, summary
    assert summary["intr_rel"] <= 1e-4 and summary["poses_abs"] <= 1e-4 * max(1.0, float(np.abs(cam[2]).max())), summary
    assert all(l["attempts"][0] == l["attempts"][1] for l in log), summary


def test_deterministic_mode_is_bit_reproducible(slice_setup, monkeypatch):
    """I3D_DETERMINISTIC=1: every sum of an outer iteration is taken in a fixed order — the gradient, the column norms, the SH Gram blocks, the camera block and the
    halo fold across workgroups in both modes; with the switch also the halo sums and the pose block INSIDE the operator pass's workgroups (halo pulled over the
    plan's lists, per-wave keyframe tables, tile_pass.hip).  Two runs of two chained iterations (Ceres' own PCG stop, every group free) from identical inputs must then agree
    bit for bit in every field — and still agree with the LDS-atomic mode (I3D_DETERMINISTIC=0) to round-off."""
    S = slice_setup; O = S["O"]; sc = S["sc"]; a0 = S["arrays"]
    cfg = helpers.gpu_cfg(bench_cfg(O, S["thres"], -1)); cfg.iterations = 2

    def run():
        ctx = helpers.gpu_context(sc, a0, S["vsh"])
        st = ctx.optimize(cfg); sdf, alb = ctx.get_grid(); cam = ctx.get_camera(); ctx.close()
        return st, sdf, alb, cam
    monkeypatch.setenv("I3D_DETERMINISTIC", "1")
    st1, s1, a1, c1 = run(); st2, s2, a2, c2 = run()
    assert np.array_equal(s1, s2) and np.array_equal(a1, a2) and all(np.array_equal(x, y) for x, y in zip(c1, c2))
    assert [(s.cost_initial, s.cost_final) for s in st1] == [(s.cost_initial, s.cost_final) for s in st2]
    assert [list(s.pcg_iterations[:s.num_attempts]) for s in st1] == [list(s.pcg_iterations[:s.num_attempts]) for s in st2]
    monkeypatch.setenv("I3D_DETERMINISTIC", "0")      # the LDS-atomic pass (the default up to round 4; still the default of a sharded run)
    st0, s0, a0_, c0 = run()
    assert [list(s.step_accepted[:s.num_attempts]) for s in st0] == [list(s.step_accepted[:s.num_attempts]) for s in st1]
    assert np.abs(s0 - s1).max() <= 1e-5 * np.abs(s1).max() and np.abs(a0_ - a1).max() <= 1e-5 * np.abs(a1).max()
    # the pulled halo on its own (I3D_HALO_PULL=1: the pose block still through LDS atomics): the same operator up to summation order
    monkeypatch.setenv("I3D_HALO_PULL", "1")
    st3, s3, a3, c3 = run()
    assert [list(s.step_accepted[:s.num_attempts]) for s in st3] == [list(s.step_accepted[:s.num_attempts]) for s in st1]
    assert np.abs(s3 - s1).max() <= 1e-5 * np.abs(s1).max() and np.abs(a3 - a1).max() <= 1e-5 * np.abs(a1).max()
