"""The oracle's trust-region controller (oracle/src/ceres_like.hpp lm_minimize) against its independent statement (tests/lm_controller_twin.py), on small NONLINEAR
problems chosen so that the twin's own trace reaches a named branch of the controller.

The problems are exponential-sum fits r(x) = A exp(s . x) - y with 12 .. 50 unknowns in blocks of sizes 1, 1, 6, 4, 5 (the parameter-block sizes of the product) and
fewer than 100 rows; residuals and the dense Jacobian reach the oracle through a C callback (orc_test_lm_callback).  Per problem the accept sequence, the CG counts,
the termination and the iteration count are EQUAL; final cost and final radius agree to rtol 1e-9 (two fp64 evaluations with different summation orders on fewer than
100 rows), the final x to rtol 1e-7.  Before that the test requires, on the twin alone, that the named branch was reached and that every discrete decision of the
trace (rho against 1e-3, the two tolerances, the CG stop ratio against 0.1) had a relative margin of at least 1e-6: no decision compared here was a coin toss."""
import numpy as np
import pytest

import lm_controller_twin as T

B12, B17, B29, B50 = [1, 1, 6, 4], [1, 1, 6, 4, 5], [1] * 8 + [6, 6, 4, 5], [1] * 20 + [6, 6, 6, 4, 4, 4]


def problem(seed, blocks, offset, noise=0.05, big=False, nan_after_move=False, exact=False):
    """fun(x, want_jacobian) of the fit, its start and its row count.  big: one unknown is 1e9 with a column of 1e-9 (|x| is large: the parameter tolerance; its column
    norm falls under the 1e-6 clamp of the LM diagonal).  nan_after_move: the Jacobian carries a NaN at every point but the start.  exact: y is the model at the start."""
    rng = np.random.default_rng(seed); n = sum(blocks); m = n + 20
    A = rng.standard_normal((m, n)); s = rng.uniform(0.5, 1.5, n); xt = rng.standard_normal(n) * 0.3
    if big:
        s[1] = 1e-9; xt[1] = 1e9
    x0 = xt + offset * rng.standard_normal(n) * ((np.arange(n) != 1) if big else 1)
    y = A @ np.exp(s * (x0 if exact else xt)) + (0 if exact else noise * rng.standard_normal(m))

    def fun(x, want_jacobian):
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(s * x); r = A @ e - y
            J = A * (s * e) if want_jacobian else None
        if want_jacobian and nan_after_move and not np.array_equal(x, x0):
            J[0, 0] = np.nan
        return r, J
    return fun, x0, m


def _rejections_then_accept(t, least=3):
    a = "".join(str(x["accepted"]) for x in t["trace"])
    return "0" * least + "1" in a


# name, problem arguments, blocks, max_iterations, stop_first, the branch the twin's trace must reach
CASES = [
    ("five rejections then accept, stop at the first success", dict(seed=0, offset=1.5), B17, 50, True, lambda t: _rejections_then_accept(t) and t["termination"] == 2),
    ("five rejections then accepts, run to the end (function tolerance)", dict(seed=2, offset=0.5), B12, 50, False,
     lambda t: _rejections_then_accept(t) and t["branches"][-1] == "function-tolerance" and t["successful"] >= 3),
    ("accepts, a run of rejections, accepts (50 unknowns)", dict(seed=1, offset=0.5), B50, 50, False, lambda t: _rejections_then_accept(t, 5) and t["trace"][0]["accepted"] == 1),
    ("function tolerance", dict(seed=1, offset=0.05), B17, 50, False, lambda t: t["branches"][-1] == "function-tolerance" and t["termination"] == 1),
    ("parameter tolerance at the first attempt", dict(seed=0, offset=0.05, big=True), B17, 50, False, lambda t: t["branches"] == ["parameter-tolerance"]),
    ("parameter tolerance after two accepts", dict(seed=2, offset=0.5, big=True), B29, 50, False, lambda t: t["branches"][-1] == "parameter-tolerance" and t["successful"] == 2),
    ("iteration limit", dict(seed=0, offset=1.5), B17, 3, False, lambda t: t["branches"][-1] == "reject+limit" and t["termination"] == 0 and t["iterations"] == 3),
    ("zero gradient at the start", dict(seed=3, offset=0.3, exact=True), B17, 50, False, lambda t: t["branches"] == ["init"] and t["iterations"] == 0 and t["termination"] == 1),
    ("five invalid steps", dict(seed=1, offset=0.05, nan_after_move=True), B17, 50, False,
     lambda t: t["branches"][-5:] == ["invalid"] * 4 + ["invalid-fail"] and t["termination"] == 3 and t["successful"] == 1),
    ("rho near 1: the 1/3 clip of the accepted radius", dict(seed=0, offset=0.05), B29, 50, True, lambda t: t["branches"] == ["accept-clip"] and t["final_radius"] > 2.99e4),
    ("rho 0.84: no clip", dict(seed=0, offset=0.5), B50, 50, True, lambda t: t["branches"] == ["accept"] and 1e4 < t["final_radius"] < 2.9e4),
]


@pytest.mark.parametrize("name,pargs,blocks,max_it,stop_first,reached", CASES, ids=[c[0] for c in CASES])
def test_oracle_controller_against_the_twin(oracle, name, pargs, blocks, max_it, stop_first, reached):
    fun, x0, m = problem(blocks=blocks, **pargs)
    assert 12 <= x0.size <= 50 and m < 100
    t = T.minimize(fun, blocks, x0, max_it, stop_first)
    print(f"\n[{name}] branches {t['branches']}, smallest decision margin {t['margin']:.3g}")
    assert reached(t), (name, t["branches"], t["termination"], t["final_radius"])
    assert t["margin"] >= 1e-6, (name, t["margin"], [(a["what"], a["margin"]) for a in t["trace"]])
    o = oracle.test_lm_callback(fun, m, blocks, x0, max_it, stop_first)
    assert o["step_accepted"] == [a["accepted"] for a in t["trace"]], (name, o["step_accepted"], [a["accepted"] for a in t["trace"]])
    assert o["cg_iterations"] == [a["cg"] for a in t["trace"]], (name, o["cg_iterations"], [a["cg"] for a in t["trace"]])
    assert (o["termination"], o["iterations"], o["successful_steps"]) == (t["termination"], t["iterations"], t["successful"]), (name, o, t["termination"], t["iterations"])
    np.testing.assert_allclose(o["initial_cost"], t["initial_cost"], rtol=1e-9)
    np.testing.assert_allclose(o["final_cost"], t["final_cost"], rtol=1e-9)
    np.testing.assert_allclose(o["final_radius"], t["final_radius"], rtol=1e-9)
    np.testing.assert_allclose(o["x"], t["x"], rtol=1e-7)


def test_scalar_controller_statements():
    """the twin's scalar controller on hand-made attempts: the two Ceres rules B.2 leaves out, and the order of the tolerances"""
    st, _ = T.init(10.0, 3, 100, 1e4)
    bad = {"model_change": -1.0, "step_norm2": 1.0, "x_norm2": 4.0, "cand_cost": 11.0, "cg_it": 3}
    for k in range(4):
        st, rec = T.decide(st, bad, k, 50)
        assert rec["what"] == "invalid" and st["nu"] == 2.0 and st["radius"] == 1e4 * 0.5 ** (k + 1)
    st5, rec = T.decide(st, bad, 4, 50)
    assert rec["what"] == "invalid-fail" and rec["final_"] == 1 and st5["termination"] == 3 and st5["radius"] == st["radius"]
    st, rec = T.decide(st, dict(bad, model_change=1.0), 4, 50)                   # a valid rejected step resets the counter
    assert rec["what"] == "reject" and st["invalid"] == 0 and st["nu"] == 4.0
    both = dict(bad, model_change=1.0, step_norm2=1e-20, cand_cost=10.0 - 1e-7)
    assert T.decide(st, both, 5, 50)[1]["what"] == "parameter-tolerance"         # B.2: the parameter tolerance is tested first
    st, rec = T.begin(dict(st, radius=9.9e-33))
    assert rec["kind"] == 2 and st["termination"] == 1 and st["done"] == 1
    assert T.begin(dict(st, radius=1e-32, done=0))[1] is None                    # below, not at, the minimum


def test_damped_blocks_statement():
    """cam_blocks / tail_diag on a block whose answer is known in closed form"""
    inv, kappa, fb = T.cam_blocks([0.0, 0.0], [0.0, 0.0, 0.0], False, 1e4)     # zero columns: S = 1, the diagonal is the 1e-6 clamp over the radius
    assert np.allclose(inv, np.eye(2) * 1e10) and not fb
    inv, _, fb = T.cam_blocks([1.0, 1.0], [1.0, 3.0, 1.0], False, 1e4)         # indefinite: the diagonal fallback
    assert fb and inv[0, 1] == 0.0 and np.isclose(inv[0, 0], 1.0 / (0.25 + 0.25e-4))
    assert np.all(T.cam_blocks([1.0, 1.0], [1.0, 0.0, 1.0], True, 1.0)[0] == 0.0)
    d2, mi = T.tail_diag([1e35, 1e-20, 4.0, 4.0], [1.0, 1.0, 0.5, 0.0], 0.5)
    assert d2[0] == np.float32(1e32) * np.float32(0.5) and d2[1] == np.float32(1e-6) * np.float32(0.5) and d2[2] == np.float32(0.5) and d2[3] == 0 and mi[3] == 0
    assert mi[2] == np.float32(1.0) / np.float32(1.5)
