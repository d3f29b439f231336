"""i3d_track_frame_sdf / i3d_fusion_track_sdf on the device, through the C ABI: the sums against the numpy statement (track_sdf_twin.py)
on the checked frames of track_sdf_cases.py, the registration against the twin, the render pose and i3d_register_points, the Huber weight, the fusion volume
against the context of its export, the status codes, the pixels that are ignored, the argument errors and what the calls must leave alone."""
import ctypes as C

import numpy as np
import pytest

import fusion_cases as FC
import helpers
import query_cases as Q
import register_cases as RC
import register_twin as RT
import track_cases as TC
import track_sdf_cases as SC
import track_sdf_twin as ST
import track_twin
from fusion_cases import fusion_frames  # noqa: F401  (fixtures)
from intrinsic3d_amd import binding as B

pytestmark = pytest.mark.gpu

VS = SC.VS
INT_STATS = ("iterations", "status", "valid_pixels", "valid", "inliers")


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


def _kw(key, cam, desc):
    return dict(desc, intr=cam["intr"], dist=cam["dist"], refined=key[2])


def _check_sums(dev, valid, usable, tw, n, what):
    assert valid == tw["valid"] and int(dev[28]) == tw["inliers"] and usable == tw["usable"], (what, valid, tw["valid"], dev[28], tw["inliers"], usable, tw["usable"])
    err = np.abs(dev - tw["sums"]); tol = n * 2.0 ** -52 * tw["abs_sums"]
    print(f"  {what}: n = {n}, usable {usable}, valid {valid}, inliers {tw['inliers']}, worst error / bound {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert np.all(err <= tol), (what, err, tol)


def _twin_start_sums(key, desc, start, st, g):
    """the twin's pass at the start pose of a traced run, about the run's pivot"""
    d = ST.default_desc(**desc)
    R, t = ST.pose_to_cw(start)
    c = st["pivot"]
    return ST.sums(Q.twin_grid(g, key[2]), st["points"], R, t - c, c, d["max_distance"], d["huber_delta"]), c


SUM_FRAMES = [("plain", "plain32", True, False), ("shifted", "dist32", True, False), ("negative", "plain32", False, False), ("plain", "px1", True, False),
              ("plain", "row65", True, False)]


@pytest.mark.parametrize("key", SUM_FRAMES, ids=lambda k: "-".join(str(x) for x in k))
def test_sums_equal_twin(contexts, key):
    """strides 1, 2 and 3 (the ragged edge), a gate of half a voxel, Huber on and off, the distorted camera, both fields, a 1 x 1 and a 65 x 1 image"""
    ctx = contexts(key[0])
    g, cam, depth, start, runs, _ = SC.checked_frame(key)
    for desc, _, st in runs:
        tw, c = _twin_start_sums(key, desc, start, st, g)
        n = st["points"].shape[0]
        dev, valid, usable = ctx.debug_track_sdf_sums(depth, start, c, **_kw(key, cam, desc))
        _check_sums(dev, valid, usable, tw, n, f"{key} {desc}")
        again = ctx.debug_track_sdf_sums(depth, start, c, **_kw(key, cam, desc))
        assert np.array_equal(dev, again[0]) and (valid, usable) == again[1:]                      # a fixed order: the same bits
        if "max_distance" in desc:
            assert 64 < tw["inliers"] < tw["valid"]                                                 # the gate cuts
        if desc.get("huber_delta", 0.0) > 0.0:
            assert (tw["weight"] < 1.0).sum() > 10                                                  # the weight acts


def test_sums_two_samples_per_lane(contexts):
    """64 x 48 = 3072 samples are 12 workgroups; a row cap of 8 makes them walk two per lane (6 workgroups of 512 samples)"""
    ctx = contexts("plain")
    L = B.load()
    key = ("plain", "plain64", True, False)
    g, cam, depth, start, runs, _ = SC.checked_frame(key)
    out = {}
    for desc, tw_pose, st in runs:
        tw, c = _twin_start_sums(key, desc, start, st, g)
        one = ctx.debug_track_sdf_sums(depth, start, c, **_kw(key, cam, desc))
        assert L.i3d_debug_register_row_cap(ctx.h, SC.ROW_CAP_P2) == 0
        try:
            two = ctx.debug_track_sdf_sums(depth, start, c, **_kw(key, cam, desc))
            again = ctx.debug_track_sdf_sums(depth, start, c, **_kw(key, cam, desc))
            if desc.get("iterations", 30) > 0:
                out["capped"] = ctx.track_frame_sdf(depth, start, **_kw(key, cam, desc))
        finally:
            assert L.i3d_debug_register_row_cap(ctx.h, 0) == 0
        _check_sums(one[0], one[1], one[2], tw, 3072, f"{desc} one per lane")
        _check_sums(two[0], two[1], two[2], tw, 3072, f"{desc} two per lane")
        assert np.array_equal(two[0], again[0]) and not np.array_equal(one[0], two[0])              # another order of summation: the cap took effect
        if desc.get("iterations", 30) > 0:
            pose1, st1 = ctx.track_frame_sdf(depth, start, **_kw(key, cam, desc))
            pose2, st2 = out["capped"]
            assert all(st1[k] == st2[k] == st[k] for k in INT_STATS) and st1["status"] == 0
            b_ang, b_tr, _ = SC.order_bar(key, 0)
            for p in (pose1, pose2):
                ang, tr = ST.pose_err(p, tw_pose, VS)
                assert ang <= b_ang and tr <= b_tr, (ang, tr, b_ang, b_tr)


def _check_against_twin(key, i, pose, st, tw_pose, tw, truth=None):
    b_ang, b_tr, _ = SC.order_bar(key, i)
    ang, tr = ST.pose_err(pose, tw_pose, VS)
    quantum = SC.translation_quantum(tw_pose)
    print(f"{key} run {i}: status {st['status']} steps {st['iterations']} (twin {tw['iterations']}); against the twin {ang:.2e} rad {tr:.2e} voxel (bar {b_ang:.1e} / "
          f"{b_tr:.1e}, one ulp of t {quantum:.1e} voxel); rms {st['rms_initial']:.3e} -> {st['rms_final']:.3e}; ratio {st['min_pivot_ratio']:.3e} "
          f"(twin {tw['min_pivot_ratio']:.3e})")
    assert all(st[k] == tw[k] for k in INT_STATS), (st, {k: tw[k] for k in INT_STATS})
    assert ang <= b_ang
    if b_tr > 1e-12 or quantum < 1e-12:                                                             # track_sdf_cases.translation_quantum
        assert tr <= b_tr
    assert abs(st["rms_initial"] - tw["rms_initial"]) <= 1e-12 * tw["rms_initial"] and abs(st["rms_final"] - tw["rms_final"]) <= 1e-6 * tw["rms_final"]
    assert abs(st["min_pivot_ratio"] - tw["min_pivot_ratio"]) <= 1e-6 * tw["min_pivot_ratio"]
    if truth is not None:
        t_ang, t_tr = ST.pose_err(pose, truth, VS)
        print(f"    against the render pose {t_ang:.3e} rad {t_tr:.3e} voxel")
        assert t_ang <= SC.TRUTH_BAR_RAD and t_tr <= SC.TRUTH_BAR_VOX


@pytest.mark.parametrize("name", RC.GRID_NAMES)
def test_registration_equals_twin_and_returns_to_the_render_pose(contexts, name):
    ctx = contexts(name)
    for key, i in [r for r in SC.TRUTH_RUNS if r[0][0] == name] + ([(("negative", "plain32", False, False), 0)] if name == "negative" else []):
        g, cam, depth, start, runs, _ = SC.checked_frame(key)
        desc, tw_pose, tw = runs[i]
        pose, st = ctx.track_frame_sdf(depth, start, **_kw(key, cam, desc))
        assert st["status"] == tw["status"] == 0 and st["rms_final"] < st["rms_initial"]
        _check_against_twin(key, i, pose, st, tw_pose, tw, truth=cam["pose"])
        pose_b, st_b = ctx.track_frame_sdf(depth, start, **_kw(key, cam, desc))
        assert np.array_equal(pose, pose_b) and st == st_b                                          # the same input gives the same bits


def test_equals_register_points_on_host_points(contexts):
    """what a caller had to do before: back-project on the host, drop the invalid pixels, invert the pose"""
    ctx = contexts("plain")
    for key in (("plain", "plain32", True, False), ("plain", "dist32", True, False)):
        g, cam, depth, start, runs, _ = SC.checked_frame(key)
        pts = SC.host_points(depth, cam)
        r_pose, r_st = ctx.register_points(pts, RT.rt_to_pose(*ST.pose_to_cw(start)))
        pose, st = ctx.track_frame_sdf(depth, start, **_kw(key, cam, runs[0][0]))
        b_ang, b_tr, _ = SC.order_bar(key, 0)
        ang, tr = ST.pose_err(pose, track_twin.cw_to_pose(*RT.pose_to_rt(r_pose)), VS)
        print(f"{key}: against register_points on {pts.shape[0]} host points {ang:.2e} rad {tr:.2e} voxel (bar {b_ang:.1e} / {b_tr:.1e})")
        assert st["status"] == r_st["status"] == 0 and st["iterations"] == r_st["iterations"] and st["valid"] == r_st["valid"] and st["inliers"] == r_st["inliers"]
        assert st["valid_pixels"] == pts.shape[0]
        assert ang <= b_ang and tr <= b_tr


def test_huber_equals_twin_in_both_modes(contexts):
    ctx = contexts("plain")
    key = ("plain", "plain32", True, True)
    g, cam, depth, start, runs, _ = SC.checked_frame(key)
    errs = []
    for i, (desc, tw_pose, tw) in enumerate(runs):
        tws, c = _twin_start_sums(key, desc, start, tw, g)
        dev, valid, usable = ctx.debug_track_sdf_sums(depth, start, c, **_kw(key, cam, desc))
        _check_sums(dev, valid, usable, tws, tw["points"].shape[0], f"corrupted {desc}")
        pose, st = ctx.track_frame_sdf(depth, start, **_kw(key, cam, desc))
        _check_against_twin(key, i, pose, st, tw_pose, tw)
        errs.append(ST.pose_err(pose, cam["pose"], VS))
    print(f"corrupted frame on the device: huber off {errs[0]}, on {errs[1]}")
    assert errs[1][0] < errs[0][0] and errs[1][1] < errs[0][1]
    # huber_delta <= 0 is off: the bits of the plain kernel
    a = ctx.track_frame_sdf(depth, start, **_kw(key, cam, dict(huber_delta=-1.0)))
    b = ctx.track_frame_sdf(depth, start, **_kw(key, cam, dict()))
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]


# ---- the fusion volume -------------------------------------------------------------------------------------------------------------------------------
def test_fusion_track_sdf(fusion_frames):
    scene, frames, _ = fusion_frames
    depth, truth = frames[1]
    start = track_twin.perturb(truth, np.random.default_rng(3), 0.5, 1.0 * VS)
    kw = dict()                                                                                     # the sphere covers about 1900 of the 96 x 72 pixels
    f = FC.fused(frames)
    try:
        before = f.track_sdf(depth, start, FC.INTR, **kw)
        s_err, e_err = TC.centre_in_camera(scene, start, truth, VS), TC.centre_in_camera(scene, before[0], truth, VS)
        print(f"fusion: {before[1]}, the sphere's centre in the camera frame: start {s_err:.3f} voxel off the integrated pose's, returned {e_err:.3f}")
        # the integrated pose's neighbourhood.  One side of a nearly round sphere leaves the rotation about its centre almost free (test_gpu_register.py), and the
        # frame carries 0.375 voxel of depth noise, so what the data pins is where the sphere sits in the camera frame: the start's offset of about a voxel must
        # shrink at least by half, and the residual must drop
        assert before[1]["status"] in (0, 1) and before[1]["iterations"] >= 1 and before[1]["inliers"] > 500
        assert s_err > 0.5 and e_err < 0.5 * s_err and before[1]["rms_final"] < before[1]["rms_initial"]
        again = f.track_sdf(depth, start, FC.INTR, **kw)
        assert np.array_equal(before[0], again[0]) and before[1] == again[1]
        f.finish(0)
        after = f.track_sdf(depth, start, FC.INTR, **kw)
        assert np.array_equal(before[0], after[0]) and before[1] == after[1]                        # finish(0) leaves the table as it was
        ctx = helpers.context_of_fusion(f, FC.VS)
        try:
            for refined in (False, True):                                                           # the volume has one field: use_refined_sdf is ignored there
                c_pose, c_st = ctx.track_frame_sdf(depth, start, intr=FC.INTR, refined=refined, **kw)
                assert np.array_equal(after[0], c_pose) and after[1] == c_st
                f_pose, f_st = f.track_sdf(depth, start, FC.INTR, refined=refined, **kw)
                assert np.array_equal(after[0], f_pose) and after[1] == f_st
            for extra in (dict(huber_delta=0.5 * VS), dict(stride=2, iterations=2), dict(stride=16)):
                a, b = f.track_sdf(depth, start, FC.INTR, **extra), ctx.track_frame_sdf(depth, start, intr=FC.INTR, refined=False, **extra)
                assert np.array_equal(a[0], b[0]) and a[1] == b[1]
        finally:
            ctx.close()
    finally:
        f.close()


# ---- statuses, ignored pixels ------------------------------------------------------------------------------------------------------------------------
def test_status_codes_and_ignored_pixels(contexts):
    ctx = contexts("plain")
    key = ("plain", "plain32", True, False)
    g, cam, depth, start, runs, _ = SC.checked_frame(key)
    grid = Q.twin_grid(g, True)
    kw = _kw(key, cam, dict())
    # status 2, the pose returned bit for bit: an all-zero depth | a frame looking into empty space
    pose, st = ctx.track_frame_sdf(np.zeros_like(depth), start, **kw)
    assert st["status"] == 2 and st["valid_pixels"] == st["valid"] == st["inliers"] == st["iterations"] == 0 and np.array_equal(pose, start)
    away = np.array(start); away[:3] = -away[:3]                                                    # some other rotation: the rays leave the stored band
    far = np.where(depth > 0, np.float32(50.0), np.float32(0.0))
    pose, st = ctx.track_frame_sdf(far, away, **kw)
    assert st["status"] == 2 and st["valid_pixels"] == int((depth > 0).sum()) and st["valid"] == 0 and np.array_equal(pose, away)
    # a budget of 0: the figures only; a budget of 1: status 1
    t0 = ST.track(grid, depth, cam["intr"], cam["dist"], start, dict(iterations=0))[1]
    pose, st = ctx.track_frame_sdf(depth, start, iterations=0, **kw)
    assert np.array_equal(pose, start) and all(st[k] == t0[k] for k in INT_STATS) and st["status"] == 1 and st["rms_initial"] == st["rms_final"]
    assert abs(st["rms_final"] - t0["rms_final"]) <= 1e-12 * t0["rms_final"]
    t1_pose, t1 = ST.track(grid, depth, cam["intr"], cam["dist"], start, dict(iterations=1))
    pose, st = ctx.track_frame_sdf(depth, start, iterations=1, **kw)
    assert all(st[k] == t1[k] for k in INT_STATS) and st["status"] == 1 and st["iterations"] == 1 and not np.array_equal(pose, start)
    ang, tr = ST.pose_err(pose, t1_pose, VS)
    assert ang <= 1e-12 and tr <= 1e-10
    # the depth range, as the twin's
    lo = float(np.median(depth[depth > 0]))
    tr_pose, trs = ST.track(grid, depth, cam["intr"], cam["dist"], start, dict(min_depth=lo, iterations=0))
    pose, st = ctx.track_frame_sdf(depth, start, min_depth=lo, iterations=0, **kw)
    assert all(st[k] == trs[k] for k in INT_STATS) and 0 < st["valid_pixels"] < int((depth > 0).sum())
    # NaN / Inf / negative depths in place of zeros change no bit
    odd = depth.copy().reshape(-1)
    zero = np.nonzero(odd == 0)[0]
    odd[zero[0::3]] = np.nan; odd[zero[1::3]] = np.inf; odd[zero[2::3]] = -1.0
    odd = odd.reshape(depth.shape)
    for desc in (dict(), dict(stride=2), dict(huber_delta=SC.HUBER)):
        a = ctx.track_frame_sdf(depth, start, **_kw(key, cam, desc))
        b = ctx.track_frame_sdf(odd, start, **_kw(key, cam, desc))
        assert a[1]["status"] == 0 and np.array_equal(a[0], b[0]) and a[1] == b[1]
    c = runs[0][2]["pivot"]
    sa = ctx.debug_track_sdf_sums(depth, start, c, **kw); sb = ctx.debug_track_sdf_sums(odd, start, c, **kw)
    assert np.array_equal(sa[0], sb[0]) and sa[1:] == sb[1:]


def test_errors(contexts, fusion_frames):
    L = B.load()
    p = B._p
    dep = np.zeros((4, 4), np.float32); pose = np.zeros(6)
    intr = [30.0, 30.0, 1.5, 1.5]
    d = B.track_sdf_desc_default(intr=intr)
    with B.Context(0) as empty:
        assert L.i3d_track_frame_sdf(empty.h, d, 4, 4, p(dep), p(pose), None) == 4
        assert "no grid" in L.i3d_last_error(empty.h).decode()
    ctx = contexts("plain")
    assert L.i3d_track_frame_sdf(ctx.h, B.track_sdf_desc_default(use_context_camera=1), 4, 4, p(dep), p(pose), None) == 4      # I3D_ERR_STATE: no camera
    assert "camera" in L.i3d_last_error(ctx.h).decode()
    _, frames, _ = fusion_frames
    f = FC.fused(frames[:1])
    try:
        models = ((lambda dd, w, h, de, po, st: L.i3d_track_frame_sdf(ctx.h, dd, w, h, de, po, st), lambda: L.i3d_last_error(ctx.h).decode()),
                  (lambda dd, w, h, de, po, st: L.i3d_fusion_track_sdf(f.h, dd, w, h, de, po, st), lambda: L.i3d_fusion_last_error(f.h).decode()))
        bad_pose = np.array([0.0, 0.0, 0.0, np.nan, 0.0, 0.0]); inf_pose = np.array([np.inf, 0.0, 0.0, 0.0, 0.0, 0.0])
        D = lambda **kw: B.track_sdf_desc_default(intr=intr, **kw)
        for call, msg in models:
            cases = [((None, 4, 4, p(dep), p(pose), None), "descriptor"), ((d, 4, 4, None, p(pose), None), "depth"), ((d, 4, 4, p(dep), None, None), "pose"),
                     ((d, 0, 4, p(dep), p(pose), None), "image size"), ((d, 4, -1, p(dep), p(pose), None), "image size"), ((d, 32769, 4, p(dep), p(pose), None), "image size"),
                     ((d, 4, 32769, p(dep), p(pose), None), "image size"),
                     ((D(stride=0), 4, 4, p(dep), p(pose), None), "stride"), ((D(stride=17), 4, 4, p(dep), p(pose), None), "stride"),
                     ((D(iterations=-1), 4, 4, p(dep), p(pose), None), "iterations"), ((D(iterations=201), 4, 4, p(dep), p(pose), None), "iterations"),
                     ((D(max_distance=0.0), 4, 4, p(dep), p(pose), None), "max_distance"), ((D(max_distance=-1.0), 4, 4, p(dep), p(pose), None), "max_distance"),
                     ((D(max_distance=float("nan")), 4, 4, p(dep), p(pose), None), "max_distance"), ((D(max_distance=float("inf")), 4, 4, p(dep), p(pose), None), "max_distance"),
                     ((D(huber_delta=float("nan")), 4, 4, p(dep), p(pose), None), "huber_delta"), ((D(huber_delta=float("inf")), 4, 4, p(dep), p(pose), None), "huber_delta"),
                     ((d, 4, 4, p(dep), p(bad_pose), None), "not finite"), ((d, 4, 4, p(dep), p(inf_pose), None), "not finite"),
                     ((B.track_sdf_desc_default(intr=[0.0, 30.0, 1.5, 1.5]), 4, 4, p(dep), p(pose), None), "focal"),
                     ((B.track_sdf_desc_default(intr=[30.0, -1.0, 1.5, 1.5]), 4, 4, p(dep), p(pose), None), "focal")]
            for args, word in cases:
                assert call(*args) == 1 and word in msg(), (word, msg())
            st = B.TrackSdfStats(); st.valid = 7; st.rms_final = 3.0
            assert call(D(iterations=200, stride=16), 4, 4, p(dep), p(pose), C.byref(st)) == 0 and st.status == 2 and st.valid == 0 and st.rms_final == 0.0
            assert call(d, 4, 4, p(dep), p(pose), None) == 0                                        # stats may be null
        assert L.i3d_fusion_track_sdf(f.h, D(use_context_camera=1), 4, 4, p(dep), p(pose), None) == 1 and "use_context_camera" in L.i3d_fusion_last_error(f.h).decode()
        s = np.zeros(29)
        assert L.i3d_debug_track_sdf_sums(ctx.h, d, 4, 4, p(dep), None, p(pose[:3].copy()), p(s), None, None) == 1
        with pytest.raises(B.I3DError) as e:
            ctx.track_frame_sdf(dep, pose, intr=intr, stride=99)
        assert "failed (1)" in str(e.value) and "stride" in str(e.value)
    finally:
        f.close()


def test_tracking_on_the_field_changes_nothing(fusion_frames):
    sc = TC.scene(seed=9)
    vs = float(sc["voxel_size"])
    rng = np.random.default_rng(11)
    sdf_r = sc["sdf"].astype(np.float64) + rng.normal(0.0, 0.05 * vs, sc["keys"].shape[0])
    cfg = B.default_config(iterations=1, thres_shell=2.0 * vs)
    start = track_twin.perturb(sc["truth"], np.random.default_rng(4), 0.3, 0.5 * vs)
    results = []
    for track in (False, True):
        ctx = TC.context(sc, sdf_refined=sdf_r)
        try:
            ctx.estimate_sh(0.05, 10.0, 2.0 * vs)
            if track:
                depth, _ = TC.view(ctx, sc, sc["truth"])
                _, st = ctx.track_frame_sdf(depth, start, use_context_camera=1, stride=2)
                assert st["valid"] > 500 and st["iterations"] >= 1
                ctx.track_frame_sdf(depth, start, intr=sc["intr"], refined=False, iterations=0, huber_delta=0.5 * vs)
            stats = ctx.optimize(cfg)
            if track:
                ctx.track_frame_sdf(depth, start, use_context_camera=1)
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
    scene, frames, _ = fusion_frames
    vols = []
    for track in (False, True):
        f = FC.fused(frames)
        try:
            if track:
                f.track_sdf(frames[1][0], frames[1][1], FC.INTR)
            f.finish(10)
            if track:
                f.track_sdf(frames[1][0], frames[1][1], FC.INTR, huber_delta=0.5 * VS)
            vols.append(f.export())
        finally:
            f.close()
    for k in ("keys", "sdf", "weight", "color"):
        assert np.array_equal(vols[0][k], vols[1][k]), k
