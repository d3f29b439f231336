"""The ray-cast tracking loop without a device: the twin (track_twin.track, track_rgbd_twin.track_rgbd) on the cases of track_loop_cases.py with an analytic
model (the bumpy sphere marched analytically, or an exact plane).  Every case's trace shows the branch the case is named for, no step of any case lies within
a factor 2 of its stop threshold (the condition test_gpu_track_loop.py asserts again on the twin runs it uses), and the shared 6x6 solve (track_twin.solve, the
statement of k_track_solve) on crafted sums: the degenerate case is defined and a system that passes every pivot test returns the bits
of the formula before that definition."""
import functools
import math

import numpy as np
import pytest

import query_twin
import register_twin as RT
import track_loop_cases as LC
import track_sdf_twin as ST
import track_twin

UPPER = track_twin.UPPER


@functools.lru_cache(maxsize=None)
def _model(name):
    wd = LC.world(name)
    return wd, LC.analytic_model(wd, LC.CASES[name]["api"] == "rgbd")


@functools.lru_cache(maxsize=None)
def _run(name):
    wd, model = _model(name)
    return LC.twin_case(name, wd, model)


@pytest.mark.parametrize("name", list(LC.CASES))
def test_trace_shows_the_branch(name):
    run = _run(name)
    st = run["stats"]
    print(name, "status", st["status"], "iterations", st["iterations"], "passes", [(p["level"], p["iterations"], p["status"]) for p in run["passes"]],
          "stop margin", LC.stop_margin(run["passes"], run["desc"]))
    LC.check_branch(name, run)
    LC.assert_stop_rule_clear(run["passes"], run["desc"])
    assert sum(len(p["steps"]) for p in run["passes"]) == sum(st["iterations"])


def test_few_inliers_coarse_succeeds_with_one_level():
    wd, model = _model("few_inliers_coarse")
    run = _run("few_inliers_coarse")
    desc = LC.descriptor("few_inliers_coarse", **LC.ONE_LEVEL)
    pose, st, passes = LC.run_twin("few_inliers_coarse", wd, run["frame"], run["start"], model, desc)
    assert st["status"] == 1 and passes[0]["inliers"] >= LC.MIN_INLIERS and st["iterations"][0] == 3 and st["rms_final"] < st["rms_initial"], st
    LC.assert_stop_rule_clear(passes, desc)


def test_photo_only_status_2_counts_photometric_samples():
    wd, model = _model("rgbd_photo_only")
    run = _run("rgbd_photo_only")
    fr = LC.starved_frame(run["frame"])
    pose, st, passes = LC.run_twin("rgbd_photo_only", wd, fr, run["start"], model, run["desc"], LC.STARVED["max_photo_residual"])
    assert st["status"] == 2 and st["inliers"] >= LC.MIN_INLIERS and 0 < st["photo_samples"] < LC.MIN_INLIERS, st
    assert pose.tobytes() == np.asarray(run["start"], np.float64).tobytes()


# ---- the solve on crafted sums ------------------------------------------------------------------------------------------------------------------------------------
def _tot(A, b=None, r2=1.0, n=1000.0):
    A = np.asarray(A, np.float64)
    return np.array([A[a, c] for a, c in UPPER] + list(np.zeros(6) if b is None else b) + [r2, n])


def _solve_before(tot):
    """the solve as it stood before the degenerate case was defined (the factorisation went on after a failing pivot): what a passing system must still return"""
    tot = [float(x) for x in tot]
    if tot[28] < track_twin.MIN_INLIERS:
        return 2, None, 0.0
    A = [[0.0] * 6 for _ in range(6)]
    for k, (a, c) in enumerate(UPPER):
        A[a][c] = A[c][a] = tot[k]
    b = tot[21:27]
    trace = A[0][0]
    for a in range(1, 6):
        trace = trace + A[a][a]
    L = [[0.0] * 6 for _ in range(6)]
    piv = [0.0] * 6
    degenerate = False
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        piv[j] = d
        if not d > 1e-12 * trace:
            degenerate = True
        L[j][j] = math.sqrt(max(d, 0.0))
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j] if L[j][j] != 0.0 else math.inf
    ratio = min(piv) / max(piv) if max(piv) > 0 else 0.0
    if degenerate:
        return 3, None, ratio
    y = [0.0] * 6
    for i in range(6):
        v = -b[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v / L[i][i]
    return None, np.array(x), ratio


def _defined(ratio):
    return isinstance(ratio, float) and math.isfinite(ratio) and 0.0 <= ratio <= 1.0


@pytest.mark.parametrize("j", range(6))
def test_solve_exact_zero_pivot(j):
    rng = np.random.default_rng(j)
    J = rng.normal(size=(200, 6)); J[:, j] = 0.0           # column j of J exactly zero: row and column j of J^T J are exact zeros
    A = J.T @ J
    st, x, ratio = track_twin.solve(_tot(A, J.T @ rng.normal(size=200)))
    assert st == 3 and x is None and ratio == 0.0
    D = np.diag([3.0, 2.0, 5.0, 1.0, 4.0, 6.0]); D[j, j] = 0.0
    assert track_twin.solve(_tot(D)) == (3, None, 0.0)
    assert track_twin.solve(_tot(np.zeros((6, 6)))) == (3, None, 0.0)          # trace 0: the first pivot fails, no pivot is > 0


def test_solve_negative_pivot():
    A = np.diag([1.0, 1.0, 2.0, 2.0, 2.0, 2.0]); A[0, 1] = A[1, 0] = 2.0      # second pivot 1 - 4 = -3
    assert track_twin.solve(_tot(A)) == (3, None, 0.0)
    A = np.diag([-1.0, 4.0, 2.0, 2.0, 2.0, 2.0])                                # the first pivot negative: no pivot > 0 up to that column
    assert track_twin.solve(_tot(A)) == (3, None, 0.0)


def test_solve_pivot_at_the_threshold():
    x = 5e-12
    while not x > 1e-12 * (5.0 + x):                       # the smallest last pivot that passes d > 1e-12 * trace with five unit pivots before it
        x = float(np.nextafter(x, np.inf))
    st, step, ratio = track_twin.solve(_tot(np.diag([1.0, 1.0, 1.0, 1.0, 1.0, x]), np.ones(6)))
    assert st is None and ratio == x and _defined(ratio) and np.all(np.isfinite(step))
    below = float(np.nextafter(x, 0.0))
    assert not below > 1e-12 * (5.0 + below)
    st, step, ratio = track_twin.solve(_tot(np.diag([1.0, 1.0, 1.0, 1.0, 1.0, below]), np.ones(6)))
    assert st == 3 and step is None and ratio == below and _defined(ratio) and ratio <= 1e-12 * (5.0 + below) / 1.0
    # the failing pivot is the largest so far: ratio 1, never above
    st, step, ratio = track_twin.solve(_tot(np.diag([1e-13, 1.0, 1.0, 1.0, 1.0, 1.0])))
    assert st == 3 and ratio == 1.0


def test_solve_inlier_floor():
    A = np.diag([3.0, 2.0, 5.0, 1.0, 4.0, 6.0])
    assert track_twin.solve(_tot(A, n=63.0)) == (2, None, 0.0)
    st, x, ratio = track_twin.solve(_tot(A, np.ones(6), n=64.0))
    assert st is None and ratio == 1.0 / 6.0 and np.allclose(x, -1.0 / np.diag(A), rtol=1e-15, atol=0.0)


def test_solve_passing_systems_keep_their_bits():
    rng = np.random.default_rng(11)
    systems = []
    for k in range(200):
        J = rng.normal(size=(80, 6)) * np.power(10.0, rng.uniform(-3, 3, 6))
        systems.append(_tot(J.T @ J, J.T @ rng.normal(size=80)))
    for name in ("one_level", "three_levels", "rgbd", "distortion_shifted"):
        systems += [np.asarray(p["sums"][:29], np.float64) for p in _run(name)["passes"] if p["sums"] is not None]
    passed = 0
    for tot in systems:
        a, b = track_twin.solve(tot), _solve_before(tot)
        assert a[0] == b[0]
        if a[0] is None:
            passed += 1
            assert a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and _defined(a[2])
    assert passed > 150
    for tot in (_tot(np.diag([1.0, 1.0, 0.0, 0.0, 1.0, 1.0])), _tot(np.diag([1.0, 4.0, 1.0, 1.0, 1.0, -1.0]))):     # degenerate: only the status is kept
        a, b = track_twin.solve(tot), _solve_before(tot)
        assert a[0] == b[0] == 3 and _defined(a[2])
    assert not _defined(_solve_before(_tot(np.diag([1.0, 1.0, 0.0, 0.0, 1.0, 1.0])))[2])                           # what the definition replaces: nan


# ---- the flat slab under the shared solve's other drivers -------------------------------------------------------------------------------------------------------
def slab_inputs():
    """the slab as a twin grid, its analytic depth frame at the true pose, the start: what register_points and track_frame_sdf get on it"""
    wd = LC.world("flat_one_level")
    sc = wd["sc"]
    grid = query_twin.Grid(sc["keys"], sc["sdf"], sc["weight"], wd["vs"], albedo=sc["albedo_true"])
    fr = LC.make_frame("flat_one_level", wd, LC.analytic_model(wd))
    return wd, grid, fr["depth"], LC.start_pose("flat_one_level", wd)


def test_slab_gradient_is_exactly_along_z():
    wd, grid, depth, start = slab_inputs()
    sc = wd["sc"]
    rng = np.random.default_rng(2)
    lo, hi = sc["keys"].min(0) + 0.01, sc["keys"].max(0) - 0.01
    x = rng.uniform(lo, hi, (5000, 3)) * wd["vs"]
    ok, _, v, fr, _ = query_twin._locate(grid, x)
    gr, _ = query_twin._gradient(v, fr)
    assert ok.all()
    assert np.all(gr[:, 0] == 0.0) and np.all(gr[:, 1] == 0.0)          # exactly zero: the corner differences along x and y are differences of equal values
    assert np.all(np.abs(gr[:, 2] + wd["vs"]) <= 4.0 * np.spacing(wd["vs"]))     # the corner differences along z are exactly -vs; the weights sum to 1 to rounding


def test_slab_is_status_3_for_the_sdf_drivers():
    wd, grid, depth, start = slab_inputs()
    pose, st = ST.track(grid, depth, wd["intr"], wd["dist"], start)
    assert st["status"] == 3 and st["iterations"] == 0 and st["inliers"] >= LC.MIN_INLIERS and pose.tobytes() == np.asarray(start, np.float64).tobytes(), st
    assert st["min_pivot_ratio"] == 0.0                                  # the third pivot (rotation about z) is an exact zero
    pts, ok, _ = ST.samples(depth, wd["intr"], wd["dist"])
    pose_cw = RT.rt_to_pose(*ST.pose_to_cw(start))
    pose, st = RT.register(grid, pts[ok], pose_cw)
    assert st["status"] == 3 and st["iterations"] == 0 and st["inliers"] >= LC.MIN_INLIERS and pose.tobytes() == np.asarray(pose_cw, np.float64).tobytes(), st
    assert st["min_pivot_ratio"] == 0.0
