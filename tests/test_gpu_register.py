"""i3d_register_points / i3d_fusion_register_points on the device, through the C ABI: the sums against the numpy statement
(register_twin.py) on the checked point sets of register_cases.py, the registration against the twin and the truth, the fusion volume against the context of its
export, the status codes, the points that are ignored, what the calls must leave alone, and the depth-frame use."""
import ctypes as C

import numpy as np
import pytest

import fusion_cases as FC
import helpers
import query_cases as Q
import register_cases as RC
import register_twin as RT
import track_cases as TC
from fusion_cases import fusion_frames  # noqa: F401  (fixtures)
from intrinsic3d_amd import binding as B, synthetic

pytestmark = pytest.mark.gpu

VS = RC.VS


@pytest.fixture(scope="module")
def contexts():
    """one context per grid of register_cases, created on first use"""
    made = {}

    def get(name):
        if name not in made:
            g = RC.grid(name)
            ctx = B.Context(0)
            ctx.set_grid(VS, g["keys"], g["sdf"], g["sdf_refined"], g["albedo"], g["weight"], g["color"])
            made[name] = ctx
        return made[name]
    yield get
    for ctx in made.values():
        ctx.close()


def _sums(ctx, pts, pose, pivot, **desc):
    L = B.load()
    d = B.register_desc_default(**desc)
    pts = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    s = np.full(29, -1.0); v = C.c_int64(-1)
    pose = np.ascontiguousarray(pose, np.float64); pivot = np.ascontiguousarray(pivot, np.float64)
    ctx._check(L.i3d_debug_register_sums(ctx.h, C.byref(d), pts.shape[0], B._p(pts), B._p(pose), B._p(pivot), B._p(s), C.byref(v)), "i3d_debug_register_sums")
    return s, int(v.value)


def _check_sums(dev, valid, tw, n):
    assert valid == tw["valid"] and int(dev[28]) == tw["inliers"], (valid, tw["valid"], dev[28], tw["inliers"])
    err = np.abs(dev - tw["sums"]); tol = n * 2.0 ** -52 * tw["abs_sums"]
    print(f"  n = {n}: valid {valid}, inliers {tw['inliers']}, worst error / bound {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert np.all(err <= tol), (err, tol)


@pytest.mark.parametrize("name", RC.GRID_NAMES)
def test_sums_equal_twin(contexts, name):
    ctx = contexts(name)
    for refined in (True, False):
        g, pts, runs = RC.checked_set(name, refined)
        grid = Q.twin_grid(g, refined)
        start = runs[0][0]
        c = runs[0][2]["pivot"]
        R, t = RT.pose_to_rt(start)
        md = RT.default_desc()["max_distance"]
        for n in RC.SIZES:
            tw = RT.sums(grid, pts[:n], R, t - c, c, md)
            dev, valid = _sums(ctx, pts[:n], start, c, refined=refined)
            _check_sums(dev, valid, tw, n)
            again, valid2 = _sums(ctx, pts[:n], start, c, refined=refined)
            assert np.array_equal(dev, again) and valid == valid2                      # a fixed order: the same bits
        tight = RT.sums(grid, pts, R, t - c, c, 0.5 * VS)                              # a gate that cuts: valid stays, inliers drop
        dev, valid = _sums(ctx, pts, start, c, refined=refined, max_distance=0.5 * VS)
        assert 64 < tight["inliers"] < tight["valid"]
        _check_sums(dev, valid, tight, RC.N_FULL)


def test_sums_two_points_per_lane(contexts):
    """a row cap of 8 makes 3000 points walk two per lane (6 workgroups of 512 points)"""
    ctx = contexts("plain")
    L = B.load()
    g, pts, runs = RC.checked_set("plain", True)
    grid = Q.twin_grid(g, True)
    start, c = runs[0][0], runs[0][2]["pivot"]
    R, t = RT.pose_to_rt(start)
    tw = RT.sums(grid, pts, R, t - c, c, RT.default_desc()["max_distance"])
    one, v1 = _sums(ctx, pts, start, c)
    assert L.i3d_debug_register_row_cap(ctx.h, 8193) == 1 and L.i3d_debug_register_row_cap(ctx.h, -1) == 1
    assert L.i3d_debug_register_row_cap(ctx.h, RC.ROW_CAP_P2) == 0
    try:
        two, v2 = _sums(ctx, pts, start, c)
        again, _ = _sums(ctx, pts, start, c)
        pose2, st2 = ctx.register_points(pts, start)
    finally:
        assert L.i3d_debug_register_row_cap(ctx.h, 0) == 0
    _check_sums(two, v2, tw, RC.N_FULL)
    assert v1 == v2 and np.array_equal(two, again)
    assert not np.array_equal(one, two)                                                # another order of summation: the cap took effect
    pose1, st1 = ctx.register_points(pts, start)
    assert st1["status"] == st2["status"] == 0 and st1["iterations"] == st2["iterations"]
    ang, tr = RT.pose_diff(pose1, pose2, VS)
    assert ang <= 1e-12 and tr <= 1e-10                                                # another order of the sums moves the pose by rounding only


@pytest.mark.parametrize("name", RC.GRID_NAMES)
def test_registration_equals_twin_and_finds_the_truth(contexts, name):
    ctx = contexts(name)
    for refined in (True, False):
        g, pts, runs = RC.checked_set(name, refined)
        truth = RC.true_pose(g)
        for k, (start, tw_pose, tw) in enumerate(runs):
            pose, st = ctx.register_points(pts, start, refined=refined)
            b_ang, b_tr, _ = RC.twin_order_bar(name, refined, k)
            ang, tr = RT.pose_diff(pose, tw_pose, VS)
            t_ang, t_tr = RT.pose_diff(pose, truth, VS)
            print(f"{name} refined={refined} start {k}: status {st['status']} steps {st['iterations']} (twin {tw['iterations']}); against the twin {ang:.2e} rad "
                  f"{tr:.2e} voxel (bar {b_ang:.1e} / {b_tr:.1e}); against the truth {t_ang:.2e} rad {t_tr:.2e} voxel; rms {st['rms_initial']:.3e} -> {st['rms_final']:.3e}; "
                  f"ratio {st['min_pivot_ratio']:.3e} (twin {tw['min_pivot_ratio']:.3e})")
            assert st["status"] == tw["status"] == 0 and st["iterations"] == tw["iterations"]
            assert st["valid"] == tw["valid"] and st["inliers"] == tw["inliers"]
            assert ang <= b_ang and tr <= b_tr
            assert t_ang <= RC.TRUTH_BAR_RAD and t_tr <= RC.TRUTH_BAR_VOX
            assert st["rms_final"] < st["rms_initial"]
            assert abs(st["rms_initial"] - tw["rms_initial"]) <= 1e-12 * tw["rms_initial"] and abs(st["min_pivot_ratio"] - tw["min_pivot_ratio"]) <= 1e-6 * tw["min_pivot_ratio"]
            pose_b, st_b = ctx.register_points(pts, start, refined=refined)
            assert np.array_equal(pose, pose_b) and st == st_b                         # the same input gives the same bits


# ---- the fusion volume -------------------------------------------------------------------------------------------------------------------------------
def _fusion_case(fusion_frames):
    """points on the fused surface (feet of the volume's own projection, moved into a frame of their own) and a perturbed start"""
    scene, frames, qpts = fusion_frames
    return scene, frames, qpts[:2000]


def _frame_and_start(scene, feet):
    truth = RT.rt_to_pose(synthetic.aa_to_rotmat(np.array([0.1, 0.2, -0.15])), scene.c.copy())
    Rt, tt = RT.pose_to_rt(truth)
    pts = (feet - tt) @ Rt
    Rd = synthetic.aa_to_rotmat(np.array([0.004, -0.006, 0.005]))
    start = RT.rt_to_pose(Rd @ Rt, Rd @ (tt - scene.c) + scene.c + np.array([0.6, -0.4, 0.5]) * VS)
    return pts, truth, start


@pytest.mark.parametrize("correct", [0, 10])
def test_fusion_registration_equals_context_registration(fusion_frames, correct):
    scene, frames, qpts = _fusion_case(fusion_frames)
    f = FC.fused(frames)
    try:
        q = f.query_points(qpts)
        feet = q["foot"][q["status"] == 3]
        assert feet.shape[0] > 500
        pts, truth, start = _frame_and_start(scene, feet)
        before = f.register_points(pts, start)
        ang, tr = RT.pose_diff(before[0], truth, VS)
        print(f"fusion: {pts.shape[0]} points, status {before[1]['status']}, {before[1]['iterations']} steps, against the truth {ang:.2e} rad {tr:.2e} voxel, "
              f"ratio {before[1]['min_pivot_ratio']:.2e}, rms {before[1]['rms_initial']:.2e} -> {before[1]['rms_final']:.2e}")
        # (one side of a nearly round sphere leaves the rotation about its centre almost free: only the residual is asserted, not the pose)
        assert before[1]["status"] in (0, 1) and before[1]["iterations"] >= 1 and before[1]["inliers"] > 500 and before[1]["rms_final"] < before[1]["rms_initial"]
        f.finish(correct)
        after = f.register_points(pts, start)
        if correct == 0:
            assert np.array_equal(before[0], after[0]) and before[1] == after[1]       # finish(0) leaves the table as it was
        ctx = helpers.context_of_fusion(f, FC.VS)
        try:
            for refined in (False, True):                                              # the volume has one field: use_refined_sdf is ignored there
                c_pose, c_st = ctx.register_points(pts, start, refined=refined)
                assert np.array_equal(after[0], c_pose) and after[1] == c_st
                f_pose, f_st = f.register_points(pts, start, refined=refined)
                assert np.array_equal(after[0], f_pose) and after[1] == f_st
            for n in (1, 63, 65, 257):                                                 # partial waves and workgroups, status 2 included
                a, b = f.register_points(pts[:n], start), ctx.register_points(pts[:n], start, refined=False)
                assert np.array_equal(a[0], b[0]) and a[1] == b[1]
        finally:
            ctx.close()
    finally:
        f.close()


# ---- statuses --------------------------------------------------------------------------------------------------------------------------------------------
def test_status_codes(contexts):
    ctx = contexts("plain")
    g, pts, runs = RC.checked_set("plain", True)
    grid = Q.twin_grid(g, True)
    start, tw_pose, tw = runs[0]
    # status 2, the pose returned unchanged bit for bit: empty space | n = 0 | 63 inliers
    pose, st = ctx.register_points(RC.empty_points(g, 500, 3), start)
    assert st["status"] == 2 and st["valid"] == 0 and st["inliers"] == 0 and st["iterations"] == 0 and np.array_equal(pose, start)
    pose, st = ctx.register_points(np.zeros((0, 3)), start)
    assert st["status"] == 2 and np.array_equal(pose, start) and st["valid"] == st["inliers"] == st["iterations"] == 0
    t63 = RT.register(grid, pts[:63], start)[1]
    pose, st = ctx.register_points(pts[:63], start)
    assert st["status"] == t63["status"] == 2 and np.array_equal(pose, start) and st["valid"] == t63["valid"] and st["inliers"] == t63["inliers"] <= 63
    # the smallest set that may step: all of its first 65 points are inliers at this start or the twin says 2 as well
    t65 = RT.register(grid, pts[:200], start)
    pose, st = ctx.register_points(pts[:200], start)
    assert st["status"] == t65[1]["status"] and st["iterations"] == t65[1]["iterations"]
    # status 1 with a budget of 1
    t1_pose, t1 = RT.register(grid, pts, start, dict(iterations=1))
    pose, st = ctx.register_points(pts, start, iterations=1)
    assert st["status"] == t1["status"] == 1 and st["iterations"] == 1 and not np.array_equal(pose, start)
    ang, tr = RT.pose_diff(pose, t1_pose, VS)
    assert ang <= 1e-12 and tr <= 1e-10
    assert st["valid"] == t1["valid"] and st["inliers"] == t1["inliers"] and abs(st["rms_final"] - t1["rms_final"]) <= 1e-9 * t1["rms_final"]
    # iterations = 0: the figures, the pose unchanged
    t0 = RT.register(grid, pts, start, dict(iterations=0))[1]
    pose, st = ctx.register_points(pts, start, iterations=0)
    assert np.array_equal(pose, start) and st["status"] == t0["status"] == 1 and st["iterations"] == 0
    assert st["valid"] == t0["valid"] and st["inliers"] == t0["inliers"] and st["rms_initial"] == st["rms_final"]
    assert abs(st["rms_final"] - t0["rms_final"]) <= 1e-12 * t0["rms_final"] and abs(st["rms_final"] - tw["rms_initial"]) <= 1e-12 * tw["rms_initial"]


def test_ignored_points_change_no_bit(contexts):
    for name in ("plain", "shifted"):
        ctx = contexts(name)
        g, pts, runs = RC.checked_set(name, True)
        start = runs[1][0]
        both = np.concatenate([pts, RC.SPECIAL])
        a = ctx.register_points(pts, start)
        b = ctx.register_points(both, start)
        assert a[1]["status"] == 0 and np.array_equal(a[0], b[0]) and a[1] == b[1]
        c = runs[1][2]["pivot"]
        sa, va = _sums(ctx, pts, start, c)
        sb, vb = _sums(ctx, both, start, c)
        assert np.array_equal(sa, sb) and va == vb
        only = ctx.register_points(RC.SPECIAL, start)
        assert only[1]["status"] == 2 and only[1]["valid"] == 0 and np.array_equal(only[0], start)


def test_registration_changes_nothing(contexts, fusion_frames):
    sc = TC.scene(seed=9)
    vs = float(sc["voxel_size"])
    rng = np.random.default_rng(11)
    sdf_r = sc["sdf"].astype(np.float64) + rng.normal(0.0, 0.05 * vs, sc["keys"].shape[0])
    cfg = B.default_config(iterations=1, thres_shell=2.0 * vs)
    near = np.abs(sc["sdf"]) < 1.5 * vs
    pts = sc["keys"][near][:3000].astype(np.float64) * vs + 0.3 * vs                    # world points inside the band
    start = np.array([0.004, -0.003, 0.002, 0.5 * vs, -0.4 * vs, 0.3 * vs])
    results = []
    for register in (False, True):
        ctx = TC.context(sc, sdf_refined=sdf_r)
        try:
            ctx.estimate_sh(0.05, 10.0, 2.0 * vs)
            if register:
                _, st = ctx.register_points(pts, start)
                assert st["valid"] > 1000 and st["iterations"] >= 1
                ctx.register_points(pts, start, refined=False, iterations=0)
            stats = ctx.optimize(cfg)
            if register:
                ctx.register_points(pts, start)
            results.append((ctx.get_grid(), ctx.export_grid(), ctx.get_camera(), stats))
        finally:
            ctx.close()
    (a0, g0, c0, s0), (a1, g1, c1, s1) = results
    for x, y in zip(a0, a1):
        assert np.array_equal(x, y)
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
    for x, y in zip(c0, c1):
        assert np.array_equal(x, y)
    for x, y in zip(s0, s1):
        for name, _ in B.IterationStats._fields_:
            if not name.startswith("time_"):
                u, v = getattr(x, name), getattr(y, name)
                assert (list(u) == list(v)) if hasattr(u, "__len__") else u == v, name
    scene, frames, qpts = _fusion_case(fusion_frames)
    vols = []
    for register in (False, True):
        f = FC.fused(frames)
        try:
            if register:
                q = f.query_points(qpts)
                p, _, start = _frame_and_start(scene, q["foot"][q["status"] == 3])
                f.register_points(p, start)
            f.finish(10)
            if register:
                f.register_points(p, start)
            vols.append(f.export())
        finally:
            f.close()
    for k in ("keys", "sdf", "weight", "color"):
        assert np.array_equal(vols[0][k], vols[1][k]), k


def test_depth_frame_registration(contexts):
    ctx = contexts("plain")
    g = RC.grid("plain")
    cam = Q.view_camera(g)
    dev = ctx.render_view(frame=-1, camera=cam, planes=("depth",))
    pts, truth, start = RC.view_case(g, dev["depth"])
    assert pts.shape[0] > 200
    pose, st = ctx.register_points(pts, start)
    ang, tr = RT.pose_diff(pose, truth, VS)
    tw_pose, tw = RT.register(Q.twin_grid(g, True), pts, start)
    print(f"view: {pts.shape[0]} points, {st['iterations']} steps, status {st['status']}, returns within {ang:.2e} rad {tr:.2e} voxel "
          f"(bars {RC.VIEW_BAR_RAD:.0e} / {RC.VIEW_BAR_VOX:.0e}); against the twin on the same points {RT.pose_diff(pose, tw_pose, VS)}")
    assert st["status"] == tw["status"] == 0 and st["iterations"] == tw["iterations"] and st["inliers"] == tw["inliers"]
    assert ang <= RC.VIEW_BAR_RAD and tr <= RC.VIEW_BAR_VOX
    assert st["rms_final"] < st["rms_initial"]


def test_errors(contexts, fusion_frames):
    L = B.load()
    p = B._p
    pts = np.zeros((4, 3)); pose = np.zeros(6)
    d = B.register_desc_default()
    with B.Context(0) as empty:
        assert L.i3d_register_points(empty.h, d, 4, p(pts), p(pose), None) == 4
        assert "no grid" in L.i3d_last_error(empty.h).decode()
    _, frames, _ = fusion_frames
    f = FC.fused(frames[:1])
    try:
        ctx = contexts("plain")
        models = ((lambda dd, n, pp, po, st: L.i3d_register_points(ctx.h, dd, n, pp, po, st), lambda: L.i3d_last_error(ctx.h).decode()),
                  (lambda dd, n, pp, po, st: L.i3d_fusion_register_points(f.h, dd, n, pp, po, st), lambda: L.i3d_fusion_last_error(f.h).decode()))
        bad_pose = np.array([0.0, 0.0, 0.0, np.nan, 0.0, 0.0]); inf_pose = np.array([np.inf, 0.0, 0.0, 0.0, 0.0, 0.0])
        for call, msg in models:
            cases = [((None, 4, p(pts), p(pose), None), "descriptor"), ((d, 4, None, p(pose), None), "points"), ((d, 4, p(pts), None, None), "pose"),
                     ((d, -1, p(pts), p(pose), None), "n must"), ((d, (1 << 27) + 1, p(pts), p(pose), None), "n must"),
                     ((B.register_desc_default(iterations=-1), 4, p(pts), p(pose), None), "iterations"), ((B.register_desc_default(iterations=201), 4, p(pts), p(pose), None), "iterations"),
                     ((B.register_desc_default(max_distance=0.0), 4, p(pts), p(pose), None), "max_distance"), ((B.register_desc_default(max_distance=-1.0), 4, p(pts), p(pose), None), "max_distance"),
                     ((B.register_desc_default(max_distance=float("nan")), 4, p(pts), p(pose), None), "max_distance"),
                     ((B.register_desc_default(max_distance=float("inf")), 4, p(pts), p(pose), None), "max_distance"),
                     ((d, 4, p(pts), p(bad_pose), None), "not finite"), ((d, 4, p(pts), p(inf_pose), None), "not finite")]
            for args, word in cases:
                assert call(*args) == 1 and word in msg(), (word, msg())
            st = B.RegisterStats(); st.valid = 7; st.rms_final = 3.0
            assert call(d, 0, None, p(pose), C.byref(st)) == 0 and st.status == 2 and st.valid == 0 and st.rms_final == 0.0      # n = 0: status 2, zero figures
            assert call(B.register_desc_default(iterations=200), 4, p(pts), p(pose), None) == 0                                    # stats may be null
        with pytest.raises(B.I3DError) as e:
            ctx.register_points(pts, pose, iterations=500)
        assert "failed (1)" in str(e.value) and "iterations" in str(e.value)
    finally:
        f.close()
