"""-m gpu: the solver's rows, normal equations, recolouring and solve against the CPU oracle OFF the zero point of the lens distortion, and at keyframes with a zero or
near-zero rotation (tests/distortion_cases.py; the input conditions are asserted on the oracle alone in test_oracle_cpu.py too).

Every scene of test_gpu_parity.py has dist = 0 and orbiting cameras: the distortion's part of k_build's chain rule (build.hip: dcr, the k3 / k4 parts of dxd_dx0 ..
dyd_dy0, c2 = 2 k4 y0 with the distorted-x quirk of camera.h:96-116, xd in the intrinsics partials) multiplies by zero there, the float observation pass, the cull bound
and k_recolor never take their Brown branch against the oracle, and the first-order branch of the angle-axis rotation (frame_math.hpp) is never assembled.  Here the same
comparisons run, case by case, with the bars of test_gpu_parity.py: structure exact, row weights 1e-5, residuals 1e-4, the 29 partials 1e-4 |J| + 2e-6 x column maximum
and 2e-4 row-relative per column group, cost 1e-5, diagonal 2e-4, gradient 2e-3 / 2e-5 max |g| entrywise and 1e-4 in the max norm, J^T J x 2e-3 / 2e-5 max |y|.  No row
is left out: the row sets must be equal."""
import numpy as np
import pytest

import distortion_cases as DC
import helpers

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=list(DC.CASES))
def case(request, oracle):
    """One case, assembled once on each side."""
    name = request.param
    sc = DC.case_scene(name)
    g, fr, arrays, vsh, thres = helpers.oracle_setup(oracle, sc)
    ocfg = helpers.oracle_cfg(oracle, thres)
    pv = oracle.ProblemView(g, fr, ocfg, sc["intr"], sc["dist"], sc["poses"], vsh, 0)
    facts = DC.input_facts(oracle, name, sc, g, fr, vsh, ocfg, pv)
    ctx = helpers.gpu_context(sc, arrays, vsh)
    try:
        ctx.debug_assemble(helpers.gpu_cfg(ocfg), 0)
        yield dict(name=name, O=oracle, sc=sc, g=g, fr=fr, arrays=arrays, vsh=vsh, thres=thres, ocfg=ocfg, pv=pv, ctx=ctx, facts=facts)
    finally:
        ctx.close(); pv.free(); g.free(); fr.free()


def _check_inputs(case):
    assert len(case["arrays"]["keys"]) == 6640
    DC.assert_inputs(case["name"], case["facts"])


def _device_row_set(gfr):
    return set((int(i), int(gfr[i, k])) for i, k in zip(*np.nonzero(gfr >= 0)))


def test_flags_and_row_structure_bit_exact(case):
    _check_inputs(case)
    pv, ctx = case["pv"], case["ctx"]
    fl = pv.flags(); gf = ctx.debug_flags()
    assert np.array_equal((gf >> 1) & 1, fl["active"])
    assert np.array_equal((gf >> 2) & 1, fl["ring_ok"])
    assert np.array_equal(((gf >> 3) & 1) ^ 1, fl["fix_sdf"])
    assert np.array_equal(((gf >> 4) & 1) ^ 1, fl["fix_alb"])
    (v, f, w, r, _), exp = DC.row_set(pv)
    gfr, gw, gr, _ = ctx.debug_eg_rows(jac=False)
    got = _device_row_set(gfr)
    print(f"\n[{case['name']}] inputs {case['facts']}; Eg rows: oracle {len(exp)}, device {len(got)}, only oracle {len(exp - got)}, only device {len(got - exp)}")
    assert got == exp, (sorted(exp - got)[:8], sorted(got - exp)[:8])
    er, es, ea = ctx.debug_reg_rows()
    v1, _, _, _ = pv.reg(1); v2, _, _, _ = pv.reg(2); v3, d3, w3, _ = pv.reg(3)
    assert set(np.nonzero(er)[0].tolist()) == set(v1.tolist())
    assert set(np.nonzero(es)[0].tolist()) == set(v2.tolist())
    assert set(zip(*[a.tolist() for a in np.nonzero(ea)])) == set(zip(v3.tolist(), d3.tolist()))
    np.testing.assert_allclose(ea[v3, d3], w3, rtol=2e-6)
    assert pv.rows == [len(v), len(v1), len(v2), len(v3)]
    assert ctx.problem_sizes()["eg"] == len(v)


def _print_figures(title, fig):
    print(f"  {title}: " + "; ".join(f"{k} {v['entry']:.3f} / {v['row']:.3f} ({v['rows']} rows)" for k, v in fig.items()))


def test_eg_weights_residuals_and_the_29_partials(case):
    """Printed per column group: worst error over tolerance of the per-entry check / of the row-relative check (the rows that check looks at)."""
    _check_inputs(case)
    pv, ctx = case["pv"], case["ctx"]
    v, f, w, r, J = pv.eg(with_jacobian=True)
    gfr, gw, gr, gJ = ctx.debug_eg_rows(jac=True)
    assert _device_row_set(gfr) == set(zip(v.tolist(), f.tolist()))          # every oracle row has its slot, and there is no other row
    slot = np.array([int(np.nonzero(gfr[vi] == fi)[0][0]) for vi, fi in zip(v, f)])
    np.testing.assert_allclose(gw[v, slot], w, rtol=1e-5)
    np.testing.assert_allclose(gr[v, slot], r, rtol=1e-4, atol=1e-9)
    Jg = gJ[v, slot]
    if np.any(case["sc"]["dist"] != 0.0):                                    # the case is off the zero point: the terms that vanish at k = 0 carry weight here
        assert np.abs(J[:, 24:29]).max(axis=0).min() > 0.0
    print(f"\n[{case['name']}] {len(v)} Eg rows; error over tolerance, per entry / row-relative")
    fig = DC.jacobian_figures(J, Jg)
    _print_figures("all rows", fig)
    figs = [("all rows", fig)]
    if case["facts"]["replaced"] is not None:                                # three keyframes out of six could hide behind the others' column maxima
        sel = np.isin(f, DC.REPLACED)
        assert sel.sum() == sum(case["facts"]["replaced"])
        fig3 = DC.jacobian_figures(J[sel], Jg[sel])
        _print_figures(f"keyframes {DC.REPLACED} alone ({int(sel.sum())} rows)", fig3)
        figs.append(("replaced keyframes", fig3))
        for k in DC.REPLACED:                                                # and each of the three branches on its own
            figk = DC.jacobian_figures(J[f == k], Jg[f == k])
            _print_figures(f"keyframe {k} alone", figk)
            figs.append((f"keyframe {k}", figk))
    for what, fg in figs:
        for group, x in fg.items():
            assert x["entry"] <= 1.0 and x["row"] < 1.0, (case["name"], what, group, x)


def test_normal_equations(case):
    _check_inputs(case)
    pv, ctx = case["pv"], case["ctx"]
    cost, g, dg, free = pv.normal_eq()
    gg, gd, gcost = ctx.debug_normal_eq()
    print(f"\n[{case['name']}] cost {abs(gcost - cost) / cost:.2e}; gradient: max-norm error {np.abs(gg - g).max() / np.abs(g).max():.2e} of max |g|; "
          f"diagonal: {np.abs(gd - dg).max() / np.abs(dg).max():.2e}; distortion entries of g {g[-5:]}, device error {np.abs(gg - g)[-5:]}")
    assert abs(gcost - cost) <= 1e-5 * cost
    np.testing.assert_allclose(gd, dg, rtol=2e-4, atol=1e-6 * dg.max())
    np.testing.assert_allclose(gg, g, rtol=2e-3, atol=2e-5 * np.abs(g).max())
    assert np.abs(gg - g).max() <= 1e-4 * np.abs(g).max()
    rng = np.random.default_rng(0)
    x = rng.normal(0, 1, g.shape) * free
    y = pv.jtj_apply(x); gy = ctx.debug_jtj_apply(x)
    np.testing.assert_allclose(gy, y, rtol=2e-3, atol=2e-5 * np.abs(y).max())


def test_recompute_colors_bit_exact_under_distortion(oracle):
    """k_recolor shares the float camera's Brown branch: the recoloured grid of the `both` case equals the oracle's byte for byte."""
    sc = DC.case_scene("both")
    g, fr, arrays, vsh, thres = helpers.oracle_setup(oracle, sc)
    assert np.any(np.abs(sc["dist"]) > DC.FLOAT_PASS_THRESHOLD)
    ctx = helpers.gpu_context(sc, arrays, vsh)
    try:
        ctx.recompute_colors(0.02, 5)
        out = ctx.export_grid()
    finally:
        ctx.close()
    oracle.recompute_colors(g, fr, sc["intr"], sc["dist"], sc["poses"], 0.02, 5)
    ref = g.export()
    changed = int(np.any(ref["color"] != arrays["color"], axis=1).sum())
    assert changed > 0.2 * len(g), changed                               # the test must exercise the recolouring
    # ... and the distortion decides colours: the oracle at zero distortion gives another grid
    g0, fr0, arrays0, _, _ = helpers.oracle_setup(oracle, sc)             # the same grid again (seeded)
    assert np.array_equal(arrays0["keys"], arrays["keys"]) and np.array_equal(arrays0["color"], arrays["color"])
    oracle.recompute_colors(g0, fr0, sc["intr"], np.zeros(5), sc["poses"], 0.02, 5)
    moved = int(np.any(g0.export()["color"] != ref["color"], axis=1).sum())
    g0.free(); fr0.free()
    diff = np.abs(out["color"].astype(int) - ref["color"].astype(int))
    print(f"\n[recolouring, both] {changed} of {len(g)} voxels change colour, {moved} differ from the recolouring at zero distortion; device differs in {int((diff > 0).sum())} bytes")
    assert np.array_equal(out["keys"], ref["keys"])
    assert diff.max() == 0, (int((diff > 0).sum()), int(diff.max()))
    assert moved > 0
    g.free(); fr.free()


def _oracle_solve(O, sc, setup, ocfg, fields=None):
    g, fr, arrays, vsh, thres = setup
    g2 = O.Grid.from_voxels(sc["voxel_size"], sc["keys"], sc["sdf"], sc["weight"], sc["color"])
    g2.clear_outside_shell(thres)
    sdf, alb = (arrays["sdf_refined"], arrays["albedo"]) if fields is None else fields
    g2.import_fields(sdf_refined=sdf, albedo=alb)
    rc, intr, dist, poses, stats = O.optimize(g2, fr, ocfg, sc["intr"], sc["dist"], sc["poses"], vsh)
    ref = g2.export(); g2.free()
    assert rc == 0
    return np.asarray(intr), np.asarray(dist), np.asarray(poses), stats, ref


@pytest.mark.parametrize("start", ["dist", "below"])
def test_optimize_started_off_the_zero_point(oracle, start):
    """Two outer iterations, every parameter group free, PCG depth pinned (as test_gpu_parity.test_optimize_matches_oracle), on the base scene, started from DIST and
    from BELOW.  BELOW lies under the float observation pass's threshold (every |k| <= 1e-5, camera.cpp:135): the first iteration is assembled on the pinhole branch,
    leaves the oracle at k = [0.042, -1.11, 3.11, -4.0e-4, 3.3e-4], and the second is assembled on the Brown branch (asserted on the oracle's own result)."""
    O = oracle
    sc = DC.scene(DC.DIST if start == "dist" else DC.BELOW)
    setup = helpers.oracle_setup(O, sc)
    g, fr, arrays, vsh, thres = setup
    ocfg = helpers.oracle_cfg(O, thres, cg_fixed_iterations=5, iterations=2)
    intr, dist, poses, stats, ref = _oracle_solve(O, sc, setup, ocfg)
    assert len(stats) == 2 and stats[0].rows[0] > DC.MIN_ROWS
    if start == "below":
        assert np.all(np.abs(sc["dist"].astype(np.float32)) <= np.float32(DC.FLOAT_PASS_THRESHOLD))
        _, k1, _, st1, _ = _oracle_solve(O, sc, setup, helpers.oracle_cfg(O, thres, cg_fixed_iterations=5, iterations=1))
        assert list(st1[0].rows) == list(stats[0].rows)
        assert np.any(np.abs(k1.astype(np.float32)) > np.float32(DC.FLOAT_PASS_THRESHOLD)), k1      # the crossing
        assert stats[1].rows[0] != stats[0].rows[0]
        print(f"\n[solve from BELOW] oracle's distortion after iteration 1 {k1}; Eg rows {stats[0].rows[0]} -> {stats[1].rows[0]}")
    ctx = helpers.gpu_context(sc, arrays, vsh)
    try:
        gst = ctx.optimize(helpers.gpu_cfg(ocfg))
        sdf, alb = ctx.get_grid(); gi, gd, gp = ctx.get_camera()
    finally:
        ctx.close()
    print(f"\n[solve from {start}] rows oracle {[list(s.rows) for s in stats]} device {[list(s.rows) for s in gst]}; "
          f"cost oracle {[(s.cost_initial, s.cost_final) for s in stats]} device {[(s.cost_initial, s.cost_final) for s in gst]}")
    assert len(gst) == len(stats)
    for so, sg in zip(stats, gst):
        assert list(so.rows) == list(sg.rows)
        assert list(so.accepted[:so.n_attempts]) == list(sg.step_accepted[:sg.num_attempts])
        assert abs(so.cost_initial - sg.cost_initial) <= 1e-4 * so.cost_initial
        assert abs(so.cost_final - sg.cost_final) <= 1e-4 * so.cost_final
    dsdf = np.abs(sdf - ref["sdf_refined"]).max(); dalb = np.abs(alb - ref["albedo"]).max()
    print(f"  sdf {dsdf / np.abs(ref['sdf_refined']).max():.2e}, albedo {dalb / np.abs(ref['albedo']).max():.2e} of the field's largest value; "
          f"intrinsics {np.abs(gi / intr - 1).max():.2e}; poses {np.abs(gp - poses).max():.2e}")
    assert dsdf <= 1e-4 * np.abs(ref["sdf_refined"]).max(), dsdf
    assert dalb <= 1e-4 * np.abs(ref["albedo"]).max(), dalb
    np.testing.assert_allclose(gi, intr, rtol=1e-4)
    np.testing.assert_allclose(gp, poses, rtol=1e-4, atol=1e-6)
    # the derived distortion bound of test_optimize_matches_oracle, unchanged: the oracle again on fields perturbed by 1e-7 relative measures the amplification of every
    # component; the device solves a problem perturbed by at most 1e-4; capped by 5e-3 |k| + 5e-4
    rng = np.random.default_rng(11); eps = 1e-7
    fields = (arrays["sdf_refined"] * (1.0 + eps * rng.standard_normal(len(arrays["sdf_refined"]))), arrays["albedo"] * (1.0 + eps * rng.standard_normal(len(arrays["albedo"]))))
    _, dist3, _, stats3, _ = _oracle_solve(O, sc, setup, ocfg, fields)
    amp = np.abs(dist3 - dist) / eps; err = np.abs(np.asarray(gd) - dist)
    tol = np.minimum(np.maximum(1e-4 * np.abs(dist), 1e-4 * amp), 5e-3 * np.abs(dist) + 5e-4) + 1e-12
    print(f"  [distortion] oracle {dist}\n  device error {err}\n  amplification (change per unit relative perturbation of the fields) {amp}\n  bound {tol}\n"
          f"  the device's error corresponds to a relative perturbation of {err / np.maximum(amp, 1e-30)} (bar: 1e-4); rows of the perturbed oracle run {[list(s.rows) for s in stats3]}")
    assert np.all(err <= tol), (err, tol)
    g.free(); fr.free()
