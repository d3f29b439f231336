"""i3d_track_frame_sdf_rgbd and its batch forms on the device, through the C ABI: the per-voxel intensity and one pass of the combined sums
against the numpy statement (track_sdf_rgbd_twin.py) on the checked frames of track_sdf_rgbd_cases.py, the registration against the twin and the render pose, the
reduction to i3d_track_frame_sdf, the smooth sphere that depth cannot pin, the batch against the single calls, what the calls must leave alone, and the errors."""
import ctypes as C

import numpy as np
import pytest

import track_sdf_cases as SC
import track_sdf_rgbd_cases as PC
import track_sdf_rgbd_twin as PT
import track_sdf_twin as ST
import track_twin
from intrinsic3d_amd import binding as B

pytestmark = pytest.mark.gpu

VS = PC.VS
INT_STATS = ("iterations", "status", "valid_pixels", "valid", "inliers", "photo_samples")
CLEAN = ("plain", "plain32", True, 0)


def _context(name, sh=True, albedo=None):
    m = PC.model(name)
    ctx = B.Context(0)
    ctx.set_grid(m["voxel_size"], m["keys"], m["sdf"], m["sdf_refined"], m["albedo"] if albedo is None else albedo, m["weight"], m["color"])
    if sh:
        ctx.set_voxel_sh(m["sh"])
    return ctx


@pytest.fixture(scope="module")
def contexts():
    """one context per model of track_sdf_rgbd_cases, with the per-voxel SH, created on first use"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = _context(name)
        return made[name]
    yield get
    for ctx in made.values():
        ctx.close()


def _kw(key, cam, desc):
    return dict(desc, intr=cam["intr"], dist=cam["dist"], refined=key[2])


# ---- 1. the intensity volume ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("refined", [True, False], ids=["refined", "fused"])
@pytest.mark.parametrize("name", PC.RC.GRID_NAMES)
def test_intensity_volume_equals_twin(contexts, name, refined):
    """the NaN pattern exactly; the values within (operations) x 2^-52 x sum |term|.  Operations of a value: 8 for the length of the gradient, 2 for a component of
    the normal, at most 5 for a basis value, the product with the coefficient, 9 sums and the product with the albedo: 26, taken as 32"""
    ctx = contexts(name)
    tw, mag = PT.voxel_intensity(PC.twin_grid(name, refined), with_terms=True)
    dev = ctx.debug_voxel_intensity(refined)
    nan = np.isnan(tw)
    assert np.array_equal(np.isnan(dev), nan) and 0 < nan.sum() < tw.size
    g = PC.model(name)
    assert nan[g["weight"] == 0.0].all()
    err = np.abs(dev[~nan] - tw[~nan]); tol = 32 * 2.0 ** -52 * mag[~nan]
    print(f"{name} refined {refined}: {tw.size} voxels, {int(nan.sum())} NaN, worst error / bound {np.max(err / tol):.3f}, worst error {err.max():.2e}")
    assert np.all(err <= tol)


# ---- 2. one pass of the sums ---------------------------------------------------------------------------------------------------------------------------------
def _check_sums(dev, valid, samples, tw, n, what):
    assert valid == tw["valid"] and int(dev[28]) == tw["inliers"] and samples == tw["samples"] == int(dev[30]), (what, valid, tw["valid"], dev[28], tw["inliers"],
                                                                                                                  samples, tw["samples"], dev[30])
    err = np.abs(dev - tw["sums"]); tol = n * 2.0 ** -52 * tw["abs_sums"]
    print(f"  {what}: n = {n}, valid {valid}, inliers {tw['inliers']}, photometric samples {samples}, worst error / bound {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert np.all(err <= tol), (what, err, tol)


SUM_FRAMES = [("plain", "plain32", True, 0), ("shifted", "dist32", True, 0), ("negative", "plain32", False, 0), ("plain", "px1", True, 0), ("plain", "row65", True, 0)]


@pytest.mark.parametrize("key", SUM_FRAMES, ids=lambda k: "-".join(str(x) for x in k))
def test_sums_equal_twin(contexts, key):
    """strides 1, 2 and 3, Huber on and off, a photo gate that cuts, geometric_weight = 0, the distorted camera on the far grid, both fields, a 1 x 1 and a 65 x 1
    image (tail lanes)"""
    ctx = contexts(key[0])
    cam, depth, lum, start, runs, _ = PC.checked_frame(key)
    for i, (desc, _, st) in enumerate(runs):
        tw, c = PC.twin_start_sums(key, i)
        n = st["points"].shape[0]
        dev, valid, samples = ctx.debug_track_sdf_rgbd_sums(depth, lum, start, c, **_kw(key, cam, desc))
        _check_sums(dev, valid, samples, tw, n, f"{key} {desc}")
        again = ctx.debug_track_sdf_rgbd_sums(depth, lum, start, c, **_kw(key, cam, desc))
        assert np.array_equal(dev, again[0]) and (valid, samples) == again[1:]                      # a fixed order: the same bits
        if tw["inliers"] >= 8:
            assert 0 < tw["samples"] < tw["inliers"]                                                # both branches run: inliers without a photometric sample
        if desc.get("max_photo_residual", 0.0) > 0.0:
            assert 0 < tw["samples"] < int(tw["rp_mask"].sum())                                     # the photo gate cuts a part
        if desc.get("geometric_weight", 1.0) == 0.0:
            plain, _ = PC.twin_start_sums(key, 0)
            assert tw["samples"] == plain["samples"] and not np.array_equal(tw["sums"][:27], plain["sums"][:27]) and tw["sums"][27] == plain["sums"][27]


def test_sums_two_samples_per_lane(contexts):
    """64 x 48 = 3072 samples are 12 workgroups; a row cap of 8 makes them walk two per lane (6 workgroups of 512 samples)"""
    ctx = contexts("plain")
    L = B.load()
    key = ("plain", "plain64", True, 0)
    cam, depth, lum, start, runs, _ = PC.checked_frame(key)
    for i, (desc, tw_pose, st) in enumerate(runs):
        tw, c = PC.twin_start_sums(key, i)
        one = ctx.debug_track_sdf_rgbd_sums(depth, lum, start, c, **_kw(key, cam, desc))
        assert L.i3d_debug_register_row_cap(ctx.h, PC.ROW_CAP_P2) == 0
        try:
            two = ctx.debug_track_sdf_rgbd_sums(depth, lum, start, c, **_kw(key, cam, desc))
            capped = ctx.track_frame_sdf_rgbd(depth, lum, start, **_kw(key, cam, desc)) if desc.get("iterations", 30) > 0 else None
        finally:
            assert L.i3d_debug_register_row_cap(ctx.h, 0) == 0
        _check_sums(one[0], one[1], one[2], tw, 3072, f"{desc} one per lane")
        _check_sums(two[0], two[1], two[2], tw, 3072, f"{desc} two per lane")
        assert not np.array_equal(one[0], two[0])                                                   # another order of summation: the cap took effect
        if capped is not None:
            free = ctx.track_frame_sdf_rgbd(depth, lum, start, **_kw(key, cam, desc))
            for pose, got in (free, capped):
                _check_against_twin(key, i, pose, got, tw_pose, st)


# ---- 3. full runs --------------------------------------------------------------------------------------------------------------------------------------------
def _check_against_twin(key, i, pose, st, tw_pose, tw, truth=None, bars=None):
    vs = PC.model(key[0])["voxel_size"]
    b_ang, b_tr, _ = PC.order_bar(key, i)
    ang, tr = ST.pose_err(pose, tw_pose, vs)
    quantum = PC.translation_quantum(tw_pose)
    print(f"{key} run {i}: status {st['status']} steps {st['iterations']} (twin {tw['status']} / {tw['iterations']}); against the twin {ang:.2e} rad {tr:.2e} voxel "
          f"(bar {b_ang:.1e} / {b_tr:.1e}, one ulp of t {quantum:.1e} voxel); rms {st['rms_initial']:.3e} -> {st['rms_final']:.3e}; photo rms "
          f"{st['photo_rms_initial']:.3e} -> {st['photo_rms_final']:.3e} on {st['photo_samples']} of {st['inliers']}; ratio {st['min_pivot_ratio']:.3e}")
    assert all(st[k] == tw[k] for k in INT_STATS), (st, {k: tw[k] for k in INT_STATS})
    assert ang <= b_ang
    if b_tr > 1e-12 or quantum < 1e-12:                                                             # track_sdf_cases.translation_quantum
        assert tr <= b_tr
    for k in ("rms_initial", "photo_rms_initial"):
        assert abs(st[k] - tw[k]) <= 1e-12 * tw[k], k
    for k in ("rms_final", "photo_rms_final", "min_pivot_ratio"):
        assert abs(st[k] - tw[k]) <= 1e-6 * tw[k], k
    if truth is not None:
        t_ang, t_tr = ST.pose_err(pose, truth, vs)
        print(f"    against the render pose {t_ang:.3e} rad {t_tr:.3e} voxel")
        assert t_ang <= bars[0] and t_tr <= bars[1]


@pytest.mark.parametrize("name", PC.RC.GRID_NAMES)
def test_registration_equals_twin_and_returns_to_the_render_pose(contexts, name):
    """status, step count and every count are the twin's - on the runs that end in the limit cycle of section 21.3 (status 1 after the whole budget) too"""
    ctx = contexts(name)
    statuses = []
    for key, i in [r for r in PC.TRUTH_RUNS if r[0][0] == name] + ([(CLEAN, 3)] if name == "plain" else []):
        cam, depth, lum, start, runs, _ = PC.checked_frame(key)
        desc, tw_pose, tw = runs[i]
        pose, st = ctx.track_frame_sdf_rgbd(depth, lum, start, **_kw(key, cam, desc))
        _check_against_twin(key, i, pose, st, tw_pose, tw, truth=cam["pose"], bars=(PC.TRUTH_BAR_RAD, PC.TRUTH_BAR_VOX))
        assert st["rms_final"] < st["rms_initial"] and st["photo_rms_final"] < st["photo_rms_initial"] and 0 < st["photo_samples"] < st["inliers"]
        pose_b, st_b = ctx.track_frame_sdf_rgbd(depth, lum, start, **_kw(key, cam, desc))
        assert np.array_equal(pose, pose_b) and st == st_b                                          # the same input gives the same bits
        statuses.append(st["status"])
    assert set(statuses) <= {0, 1}


# ---- 4. the reduction ----------------------------------------------------------------------------------------------------------------------------------------
def test_without_photo_weight_it_is_track_frame_sdf_byte_for_byte():
    """photo_weight = 0, geometric_weight = 1 on a context without SH: the pose and every base figure of i3d_track_frame_sdf, in the batch too"""
    for name, skey in (("plain", ("plain", "plain32", True, False)), ("shifted", ("shifted", "dist32", True, False)), ("plain", ("plain", "plain32", True, True))):
        ctx = _context(name, sh=False)
        try:
            g, cam, depth, start, runs, _ = SC.checked_frame(skey)
            lum = np.full(depth.shape, 0.5, np.float32)
            for desc, _, _ in runs:
                kw = dict(desc, intr=cam["intr"], dist=cam["dist"], refined=skey[2])
                a_pose, a = ctx.track_frame_sdf(depth, start, **kw)
                b_pose, b = ctx.track_frame_sdf_rgbd(depth, lum, start, photo_weight=0.0, geometric_weight=1.0, **kw)
                assert a_pose.tobytes() == b_pose.tobytes(), (skey, desc)
                for k in a:
                    assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (skey, desc, k, a[k], b[k])
                assert (b["photo_samples"], b["photo_rms_initial"], b["photo_rms_final"]) == (0, 0.0, 0.0)
                out, st = ctx.track_frames_sdf_rgbd(np.stack([depth, depth]), np.stack([lum, lum]), np.stack([start, start]), photo_weight=0.0, **kw)
                assert out[1].tobytes() == a_pose.tobytes() and st[1] == b and st[0] == b
            with pytest.raises(B.I3DError) as e:                                                    # and with a photo weight the missing SH is an error
                ctx.track_frame_sdf_rgbd(depth, lum, start, intr=cam["intr"], dist=cam["dist"])
            assert "failed (4)" in str(e.value) and "SH" in str(e.value)
        finally:
            ctx.close()


# ---- 5. colour pins what depth cannot ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", PC.SMOOTH_FRAMES, ids=lambda k: f"start{k[3]}")
def test_colour_pins_what_depth_cannot(contexts, key):
    ctx = contexts("smooth")
    vs = PC.model("smooth")["voxel_size"]
    cam, depth, lum, start, runs, _ = PC.checked_frame(key)
    (d_desc, d_tw_pose, d_tw), (c_desc, c_tw_pose, c_tw) = runs
    s_ang, _ = ST.pose_err(start, cam["pose"], vs)
    pose_d, st_d = ctx.track_frame_sdf_rgbd(depth, lum, start, **_kw(key, cam, d_desc))
    _check_against_twin(key, 0, pose_d, st_d, d_tw_pose, d_tw)
    d_ang, _ = ST.pose_err(pose_d, cam["pose"], vs)
    assert d_ang >= s_ang and st_d["photo_samples"] == 0                                            # depth alone leaves the rotation where it was, or worse
    pose_c, st_c = ctx.track_frame_sdf_rgbd(depth, lum, start, **_kw(key, cam, c_desc))
    _check_against_twin(key, 1, pose_c, st_c, c_tw_pose, c_tw, truth=cam["pose"], bars=(PC.SMOOTH_BAR_RAD, PC.SMOOTH_BAR_VOX))
    assert st_c["status"] == 0 and st_c["min_pivot_ratio"] > 10.0 * st_d["min_pivot_ratio"]


# ---- 6. the batch --------------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b, what):
    """pose bytes and every field of the stats"""
    assert np.asarray(a[0], np.float64).tobytes() == np.asarray(b[0], np.float64).tobytes(), (what, a[0], b[0])
    assert set(a[1]) == set(b[1]) == {k for k, _ in B.TrackSdfStats._fields_} | {"photo_samples", "photo_rms_initial", "photo_rms_final"}
    for k in a[1]:
        assert np.float64(a[1][k]).tobytes() == np.float64(b[1][k]).tobytes(), (what, k, a[1][k], b[1][k])


def _five(ctx):
    """(camera, depths, lums, poses) of five frames: the checked frame from its start | from the pose its own call returns (done after one step while others are
    live) | an all-zero depth | the frame from another start | the frame under a brighter image"""
    cam, depth, lum, start, runs, _ = PC.checked_frame(CLEAN)
    solved, st = ctx.track_frame_sdf_rgbd(depth, lum, start, **_kw(CLEAN, cam, dict()))
    assert st["status"] == 0 and st["iterations"] > 1
    other = track_twin.perturb(cam["pose"], np.random.default_rng(31), 0.3, 0.6 * VS)
    depths = np.stack([depth, depth, np.zeros_like(depth), depth, depth]).astype(np.float32)
    lums = np.stack([lum, lum, lum, lum, lum + np.float32(0.01)]).astype(np.float32)
    poses = np.stack([start, solved, start, other, start])
    return cam, depths, lums, poses


@pytest.mark.parametrize("desc", [dict(), dict(stride=2, huber_delta=PC.HUBER), dict(iterations=2, max_photo_residual=0.02)], ids=["default", "stride2-huber", "two-steps-gated"])
def test_a_batch_equals_the_single_calls_bit_for_bit(contexts, desc):
    ctx = contexts("plain")
    cam, depths, lums, poses = _five(ctx)
    kw = _kw(CLEAN, cam, desc)
    one = [ctx.track_frame_sdf_rgbd(depths[i], lums[i], poses[i], **kw) for i in range(5)]
    print("; ".join(f"frame {i}: status {s['status']} steps {s['iterations']} inliers {s['inliers']} samples {s['photo_samples']}" for i, (_, s) in enumerate(one)))
    try:
        for n in (1, 2, 0):                                                                         # chunks of 1, of 2 (2 + 2 + 1) and the default rule
            ctx.debug_track_batch_frames(n)
            out, st = ctx.track_frames_sdf_rgbd(depths, lums, poses, **kw)
            assert out.shape == (5, 6) and len(st) == 5
            for i in range(5):
                _same((out[i], st[i]), one[i], f"{desc} frame {i}, chunks of {n}")
    finally:
        ctx.debug_track_batch_frames(0)
    assert one[2][1]["status"] == 2 and one[2][1]["valid_pixels"] == 0 and np.array_equal(one[2][0], poses[2])          # the pose untouched
    assert one[0][1]["photo_samples"] > 0 and one[4][1]["photo_rms_initial"] > one[0][1]["photo_rms_initial"]
    if not desc:
        assert one[1][1]["status"] == 0 and one[1][1]["iterations"] == 1 and all(one[i][1]["iterations"] > 1 for i in (0, 3, 4))


def test_keyframes():
    """the resident depth and luminance of a level, no upload: i3d_track_frames_sdf_rgbd's result on the images i3d_get_frame_image returns"""
    cam, depth, lum, start, _, _ = PC.checked_frame(CLEAN)
    rng = np.random.default_rng(21)
    kf_poses = np.stack([np.asarray(cam["pose"], np.float64), start, track_twin.perturb(cam["pose"], rng, 0.8, 1.5 * VS)])
    ctx = _context("plain")
    try:
        frames = []
        for p in kf_poses:
            deps, lums = [], []
            for level in (0, 1):
                w, h = cam["width"] >> level, cam["height"] >> level
                out = ctx.render_view(frame=-1, planes=("depth", "intensity"), camera=dict(width=w, height=h, intr=np.asarray(cam["intr"]) / 2 ** level, dist=cam["dist"], pose=p))
                deps.append(np.ascontiguousarray(out["depth"], np.float32).reshape(h, w)); lums.append(np.ascontiguousarray(out["intensity"], np.float32).reshape(h, w))
            frames.append(dict(lum=lums, depth=deps))
        ctx.set_frames(frames, 2)
        ctx.set_camera(cam["intr"], cam["dist"], kf_poses)
        starts = np.stack([track_twin.perturb(p, np.random.default_rng(22 + i), 0.4, 0.8 * VS) for i, p in enumerate(kf_poses)])
        before = ctx.get_camera()
        for level in (0, 1):
            w, h = cam["width"] >> level, cam["height"] >> level
            images = [ctx.get_frame_image(f, level, w, h) for f in range(3)]
            ref = ctx.track_frames_sdf_rgbd(np.stack([im[1] for im in images]), np.stack([im[0] for im in images]), starts, intr=np.asarray(cam["intr"]) / 2 ** level,
                                            dist=cam["dist"])
            out, st = ctx.track_keyframes_sdf_rgbd(starts, level=level)
            print(f"level {level}: " + "; ".join(f"status {s['status']} steps {s['iterations']} inliers {s['inliers']} samples {s['photo_samples']}" for s in st))
            for f in range(3):
                _same((out[f], st[f]), (ref[0][f], ref[1][f]), f"level {level} keyframe {f}")
            if level == 0:
                assert all(s["iterations"] >= 1 and s["photo_samples"] > 0 for s in st), st
            out, st = ctx.track_keyframes_sdf_rgbd(starts[[2, 0]], level=level, frames=[2, 0])
            _same((out[0], st[0]), (ref[0][2], ref[1][2]), f"level {level} frames=[2, 0] first")
            _same((out[1], st[1]), (ref[0][0], ref[1][0]), f"level {level} frames=[2, 0] second")
        for x, y in zip(before, ctx.get_camera()):
            assert x.tobytes() == y.tobytes()
    finally:
        ctx.close()


# ---- 7. state ------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_call_changes_nothing_and_sees_the_current_fields():
    cam, depth, lum, start, runs, _ = PC.checked_frame(CLEAN)
    kw = _kw(CLEAN, cam, dict())
    m = PC.model("plain")
    other = m["albedo"] * (1.0 + 0.3 * np.sin(np.arange(m["albedo"].size) * 0.37))
    ctx = _context("plain")
    try:
        ctx.set_frames([dict(lum=[lum], depth=[depth])], 1)
        ctx.set_camera(cam["intr"], cam["dist"], np.asarray(cam["pose"], np.float64)[None])
        before = (ctx.export_grid(), ctx.get_voxel_sh(), ctx.get_camera())
        first = ctx.track_frame_sdf_rgbd(depth, lum, start, **kw)
        ctx.track_frames_sdf_rgbd(np.stack([depth, depth]), np.stack([lum, lum]), np.stack([start, start]), stride=2, **kw)
        ctx.track_keyframes_sdf_rgbd(start[None], huber_delta=PC.HUBER)
        ctx.debug_voxel_intensity(False)
        after = (ctx.export_grid(), ctx.get_voxel_sh(), ctx.get_camera())
        for k in before[0]:
            assert np.array_equal(before[0][k], after[0][k]), k
        assert np.array_equal(before[1], after[1]) and all(x.tobytes() == y.tobytes() for x, y in zip(before[2], after[2]))
        ctx.update_grid(albedo=other)                                                               # no stale volume: the call after it reads the new albedo
        moved = ctx.track_frame_sdf_rgbd(depth, lum, start, **kw)
        fresh_ctx = _context("plain", albedo=other)
        try:
            fresh = fresh_ctx.track_frame_sdf_rgbd(depth, lum, start, **kw)
        finally:
            fresh_ctx.close()
        _same(moved, fresh, "after update_grid")
        assert moved[1]["photo_rms_initial"] != first[1]["photo_rms_initial"] and moved[0].tobytes() != first[0].tobytes()
    finally:
        ctx.close()


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------------------------------
def test_errors(contexts):
    L = B.load()
    p = B._p
    dep = np.zeros((4, 4), np.float32); lum = np.zeros((4, 4), np.float32); pose = np.zeros(6)
    intr = [30.0, 30.0, 1.5, 1.5]
    D = lambda **kw: B.track_sdf_rgbd_desc_default(intr=intr, **kw)  # noqa: E731
    d = D()
    ctx = contexts("plain")
    msg = lambda: L.i3d_last_error(ctx.h).decode()  # noqa: E731
    nan, inf = float("nan"), float("inf")
    bad_pose = np.array([0.0, 0.0, 0.0, nan, 0.0, 0.0])
    cases = [((None, 4, 4, p(dep), p(lum), p(pose), None), "descriptor"), ((d, 4, 4, None, p(lum), p(pose), None), "depth"), ((d, 4, 4, p(dep), None, p(pose), None), "luminance"),
             ((d, 4, 4, p(dep), p(lum), None, None), "pose"), ((d, 0, 4, p(dep), p(lum), p(pose), None), "image size"), ((d, 4, 32769, p(dep), p(lum), p(pose), None), "image size"),
             ((D(stride=0), 4, 4, p(dep), p(lum), p(pose), None), "stride"), ((D(stride=17), 4, 4, p(dep), p(lum), p(pose), None), "stride"),
             ((D(iterations=-1), 4, 4, p(dep), p(lum), p(pose), None), "iterations"), ((D(iterations=201), 4, 4, p(dep), p(lum), p(pose), None), "iterations"),
             ((D(max_distance=0.0), 4, 4, p(dep), p(lum), p(pose), None), "max_distance"), ((D(max_distance=nan), 4, 4, p(dep), p(lum), p(pose), None), "max_distance"),
             ((D(huber_delta=inf), 4, 4, p(dep), p(lum), p(pose), None), "huber_delta"), ((d, 4, 4, p(dep), p(lum), p(bad_pose), None), "not finite"),
             ((B.track_sdf_rgbd_desc_default(intr=[0.0, 30.0, 1.5, 1.5]), 4, 4, p(dep), p(lum), p(pose), None), "focal"),
             ((D(geometric_weight=-1.0), 4, 4, p(dep), p(lum), p(pose), None), "weights"), ((D(photo_weight=-0.1), 4, 4, p(dep), p(lum), p(pose), None), "weights"),
             ((D(geometric_weight=nan), 4, 4, p(dep), p(lum), p(pose), None), "weights"), ((D(photo_weight=inf), 4, 4, p(dep), p(lum), p(pose), None), "weights"),
             ((D(geometric_weight=0.0, photo_weight=0.0), 4, 4, p(dep), p(lum), p(pose), None), "both weights"),
             ((D(max_photo_residual=nan), 4, 4, p(dep), p(lum), p(pose), None), "max_photo_residual"), ((D(max_photo_residual=inf), 4, 4, p(dep), p(lum), p(pose), None), "max_photo_residual")]
    for args, word in cases:
        st = B.TrackSdfRgbdStats(); st.photo_samples = 7; st.base.valid = 9
        po = args[5]
        keep = None if po is None else np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_double)), (6,)).copy()
        a = args[:6] + (C.byref(st),)
        assert L.i3d_track_frame_sdf_rgbd(ctx.h, *a) == 1 and word in msg(), (word, msg())
        assert st.photo_samples == 7 and st.base.valid == 9                                         # the outputs untouched
        if keep is not None:
            assert np.array_equal(np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_double)), (6,)), keep, equal_nan=True)
        deps = p(dep) if args[3] is not None else None
        lums = p(lum) if args[4] is not None else None
        assert L.i3d_track_frames_sdf_rgbd(ctx.h, args[0], 1, args[1], args[2], deps, lums, po, C.cast(C.byref(st), C.c_void_p)) == 1 and st.photo_samples == 7, word
    assert L.i3d_track_frame_sdf_rgbd(ctx.h, B.track_sdf_rgbd_desc_default(use_context_camera=1), 4, 4, p(dep), p(lum), p(pose), None) == 4 and "camera" in msg()
    with B.Context(0) as empty:
        assert L.i3d_track_frame_sdf_rgbd(empty.h, d, 4, 4, p(dep), p(lum), p(pose), None) == 4 and "no grid" in L.i3d_last_error(empty.h).decode()
        assert L.i3d_debug_voxel_intensity(empty.h, 1, p(np.zeros(4))) == 4
    no_sh = _context("plain", sh=False)
    try:
        st = B.TrackSdfRgbdStats(); st.photo_samples = 7
        for call in (lambda: L.i3d_track_frame_sdf_rgbd(no_sh.h, d, 4, 4, p(dep), p(lum), p(pose), C.byref(st)),
                     lambda: L.i3d_track_frames_sdf_rgbd(no_sh.h, d, 1, 4, 4, p(dep), p(lum), p(pose), C.cast(C.byref(st), C.c_void_p)),
                     lambda: L.i3d_debug_voxel_intensity(no_sh.h, 1, p(np.zeros(no_sh.grid_info()[0])))):
            assert call() == 4 and "per-voxel SH" in L.i3d_last_error(no_sh.h).decode() and st.photo_samples == 7
        assert L.i3d_track_keyframes_sdf_rgbd(no_sh.h, B.track_sdf_rgbd_desc_default(use_context_camera=1), 0, 1, None, p(pose), None) == 4       # no keyframes
        assert L.i3d_track_frame_sdf_rgbd(no_sh.h, D(photo_weight=0.0), 4, 4, p(dep), p(lum), p(pose), C.byref(st)) == 0 and st.base.status == 2 and st.photo_samples == 0
    finally:
        no_sh.close()
    # a frame without data: status 2, the figures zero; stats may be null; the batch of none is a no-op
    st = B.TrackSdfRgbdStats(); st.base.valid = 7; st.photo_rms_final = 3.0
    assert L.i3d_track_frame_sdf_rgbd(ctx.h, D(iterations=200, stride=16), 4, 4, p(dep), p(lum), p(pose), C.byref(st)) == 0
    assert st.base.status == 2 and st.base.valid == 0 and st.photo_rms_final == 0.0
    assert L.i3d_track_frame_sdf_rgbd(ctx.h, d, 4, 4, p(dep), p(lum), p(pose), None) == 0
    assert L.i3d_track_frames_sdf_rgbd(ctx.h, d, 0, 4, 4, None, None, None, None) == 0 and L.i3d_track_frames_sdf_rgbd(ctx.h, d, -1, 4, 4, p(dep), p(lum), p(pose), None) == 1
    s = np.zeros(31)
    assert L.i3d_debug_track_sdf_rgbd_sums(ctx.h, d, 4, 4, p(dep), p(lum), None, p(pose[:3].copy()), p(s), None, None) == 1
    assert L.i3d_debug_voxel_intensity(ctx.h, 1, None) == 1
    with pytest.raises(B.I3DError) as e:
        ctx.track_frame_sdf_rgbd(dep, lum, pose, intr=intr, photo_weight=-1.0)
    assert "failed (1)" in str(e.value) and "weights" in str(e.value)
    # geometric_weight = 0: status 2 goes by the photometric samples (fewer than 64 here although the inliers are many)
    cam, depth, lum32, start, runs, _ = PC.checked_frame(CLEAN)
    pose_g, st_g = ctx.track_frame_sdf_rgbd(depth, lum32, start, geometric_weight=0.0, max_photo_residual=0.001, **_kw(CLEAN, cam, dict()))
    assert st_g["status"] == 2 and st_g["inliers"] > 64 > st_g["photo_samples"] and np.array_equal(pose_g, start)
