"""i3d_track_frames_sdf / i3d_track_keyframes_sdf on the device: a frame's result in a batch is i3d_track_frame_sdf's for that frame, bit for
bit - the pose bytes and every field of the stats - whatever its companions and however the batch is cut into chunks; the keyframe call reads the resident depth
under the level's camera; the errors, the no-ops and what the calls must leave alone.  The frames are the checked frames of track_sdf_cases.py."""
import ctypes as C

import numpy as np
import pytest

import query_cases as Q
import register_cases as RC
import track_cases as TC
import track_sdf_cases as SC
import track_sdf_twin as ST
import track_twin
from intrinsic3d_amd import binding as B

pytestmark = pytest.mark.gpu

VS = SC.VS
INT_STATS = ("iterations", "status", "valid_pixels", "valid", "inliers")
CLEAN = ("plain", "plain32", True, False)
CORRUPTED = ("plain", "plain32", True, True)
# the descriptors of the six-frame batch; the first three are runs 0, 1 and 4 of the clean checked frame
DESCS = {"stride1": dict(stride=1), "stride2": dict(stride=2), "huber": dict(huber_delta=SC.HUBER), "two_steps": dict(iterations=2)}
TWIN_RUN = {"stride1": 0, "stride2": 1, "huber": 4}


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


def _six():
    """(camera, depths [6, 24, 32], start poses [6, 6]): the clean checked frame from its start pose | the same depth from the render pose itself | the corrupted
    checked frame | an all-zero plane | a plane with fewer than 64 usable pixels | the clean frame again"""
    g, cam, clean, start, _, _ = SC.checked_frame(CLEAN)
    _, _, bad, bad_start, _, _ = SC.checked_frame(CORRUPTED)
    few = clean.copy().reshape(-1)
    few[np.nonzero(few > 0)[0][40:]] = 0.0
    few = few.reshape(clean.shape)
    assert 0 < int((few > 0).sum()) < 64
    depths = np.stack([clean, clean, bad, np.zeros_like(clean), few, clean]).astype(np.float32)
    poses = np.stack([start, np.asarray(cam["pose"], np.float64), bad_start, start, start, start])
    return cam, depths, poses


def _kw(cam, desc, refined=True):
    return dict(desc, intr=cam["intr"], dist=cam["dist"], refined=refined)


def _singles(ctx, depths, poses, kw):
    return [ctx.track_frame_sdf(depths[i], poses[i], **kw) for i in range(len(depths))]


def _same(a, b, what):
    """pose bytes and every field of the stats"""
    assert np.asarray(a[0], np.float64).tobytes() == np.asarray(b[0], np.float64).tobytes(), (what, a[0], b[0])
    assert set(a[1]) == set(b[1]) == {k for k, _ in B.TrackSdfStats._fields_}
    for k in a[1]:
        assert np.float64(a[1][k]).tobytes() == np.float64(b[1][k]).tobytes(), (what, k, a[1][k], b[1][k])


def _batch(ctx, depths, poses, kw):
    out, st = ctx.track_frames_sdf(depths, poses, **kw)
    assert out.shape == (len(depths), 6) and len(st) == len(depths)
    return [(out[i], st[i]) for i in range(len(depths))]


@pytest.mark.parametrize("name", list(DESCS))
def test_a_batch_equals_the_single_calls_bit_for_bit(contexts, name):
    ctx = contexts("plain")
    cam, depths, poses = _six()
    kw = _kw(cam, DESCS[name])
    one = _singles(ctx, depths, poses, kw)
    got = _batch(ctx, depths, poses, kw)
    print(f"{name}: " + "; ".join(f"frame {i}: status {s['status']} steps {s['iterations']} inliers {s['inliers']}" for i, (_, s) in enumerate(one)))
    for i in range(6):
        _same(got[i], one[i], f"{name} frame {i}")
    # the frames are what the case says they are
    assert one[3][1]["status"] == 2 and one[3][1]["valid_pixels"] == 0 and np.array_equal(got[3][0], poses[3])
    assert one[4][1]["status"] == 2 and 0 < one[4][1]["valid_pixels"] < 64 and np.array_equal(got[4][0], poses[4])
    if name == "two_steps":                                 # the budget runs out on some frames while others are already done
        assert one[0][1]["status"] == 1 and one[0][1]["iterations"] == 2 and {one[3][1]["iterations"], one[4][1]["iterations"]} == {0}
    else:
        assert all(one[i][1]["status"] == 0 for i in (0, 1, 2, 5))
        assert len({one[i][1]["iterations"] for i in (0, 1, 2)}) > 1                               # the frames finish at different passes
    # the clean frame against the numpy statement, so that the case does not rest on the single-frame call alone
    g, _, clean, start, runs, _ = SC.checked_frame(CLEAN)
    if name in TWIN_RUN:
        desc, tw_pose, tw = runs[TWIN_RUN[name]]
        assert desc == DESCS[name]
        b_ang, b_tr, _ = SC.order_bar(CLEAN, TWIN_RUN[name])
    else:                                                   # no recorded run: the twin on the spot, and order_bar's own rule for the bar
        grid = Q.twin_grid(g, True)
        tw_pose, tw = ST.track(grid, clean, cam["intr"], cam["dist"], start, DESCS[name])
        seq, _ = ST.track(grid, clean, cam["intr"], cam["dist"], start, DESCS[name], order="sequential")
        o_ang, o_tr = ST.pose_err(seq, tw_pose, VS)
        b_ang, b_tr = max(100.0 * o_ang, 1e-12), max(100.0 * o_tr, 1e-12)
    ang, tr = ST.pose_err(got[0][0], tw_pose, VS)
    print(f"{name}: the clean frame in the batch against the twin {ang:.2e} rad {tr:.2e} voxel (bar {b_ang:.1e} / {b_tr:.1e})")
    assert all(got[0][1][k] == tw[k] for k in INT_STATS), (got[0][1], {k: tw[k] for k in INT_STATS})
    assert ang <= b_ang and tr <= b_tr


def test_companions_do_not_matter(contexts):
    ctx = contexts("plain")
    cam, depths, poses = _six()
    for name in ("stride1", "two_steps"):
        kw = _kw(cam, DESCS[name])
        full = _batch(ctx, depths, poses, kw)
        for i in range(6):                                  # each frame alone
            _same(_batch(ctx, depths[i:i + 1], poses[i:i + 1], kw)[0], full[i], f"{name} frame {i} alone")
        rev = _batch(ctx, depths[::-1], poses[::-1], kw)
        for i in range(6):
            _same(rev[5 - i], full[i], f"{name} frame {i} reversed")
        order = [0, 2, 2, 1, 4, 3, 5]                       # one frame listed twice
        twice = _batch(ctx, depths[order], poses[order], kw)
        for j, i in enumerate(order):
            _same(twice[j], full[i], f"{name} frame {i} at {j}")


def test_chunks_do_not_matter(contexts):
    ctx = contexts("plain")
    cam, depths, poses = _six()
    for name in ("stride2", "huber", "two_steps"):
        kw = _kw(cam, DESCS[name])
        full = _batch(ctx, depths, poses, kw)
        try:
            for n in (2, 4):                                # 2 + 2 + 2, then 4 + 2
                ctx.debug_track_batch_frames(n)
                cut = _batch(ctx, depths, poses, kw)
                for i in range(6):
                    _same(cut[i], full[i], f"{name} frame {i}, chunks of {n}")
        finally:
            ctx.debug_track_batch_frames(0)
        again = _batch(ctx, depths, poses, kw)
        for i in range(6):
            _same(again[i], full[i], f"{name} frame {i} after the reset")


def test_single_calls_around_a_batch_are_a_fresh_contexts():
    """every form runs through one scratch and one staging area: a single call before a batch in chunks of two, the same call after it and a call on a 12 x 16
    crop (a smaller layout over what the batch left) each return the bytes of that call on a context that has done nothing else"""
    cam, depths, poses = _six()
    kw = _kw(cam, DESCS["stride1"])
    crop = np.ascontiguousarray(depths[0][:12, :16])
    g = RC.grid("plain")

    def context():
        ctx = B.Context(0)
        ctx.set_grid(VS, g["keys"], g["sdf"], g["sdf_refined"], g["albedo"], g["weight"], g["color"])
        return ctx

    fresh = []
    for depth in (depths[0], crop):
        with context() as ctx:
            fresh.append(ctx.track_frame_sdf(depth, poses[0], **kw))
    assert fresh[0][1]["status"] == 0 and fresh[0][1]["iterations"] >= 1 and 0 < fresh[1][1]["valid_pixels"] < fresh[0][1]["valid_pixels"]
    with context() as ctx:
        _same(ctx.track_frame_sdf(depths[0], poses[0], **kw), fresh[0], "before the batch")
        ctx.debug_track_batch_frames(2)
        got = _batch(ctx, depths, poses, kw)
        _same(got[0], fresh[0], "in the batch")
        _same(ctx.track_frame_sdf(depths[0], poses[0], **kw), fresh[0], "after the batch")
        _same(ctx.track_frame_sdf(crop, poses[0], **kw), fresh[1], "the crop after the batch")


def test_two_samples_per_lane(contexts):
    """64 x 48 = 3072 samples are 12 workgroups; a row cap of 8 makes them walk two per lane, in the batch as in the single call"""
    ctx = contexts("plain")
    L = B.load()
    key = ("plain", "plain64", True, False)
    g, cam, depth, start, runs, _ = SC.checked_frame(key)
    kw = _kw(cam, dict())
    depths = np.stack([depth, depth, np.where(np.arange(48)[:, None] < 24, depth, np.float32(0.0))]).astype(np.float32)
    poses = np.stack([start, np.asarray(cam["pose"], np.float64), start])
    free = _singles(ctx, depths, poses, kw)
    assert L.i3d_debug_register_row_cap(ctx.h, SC.ROW_CAP_P2) == 0
    try:
        one = _singles(ctx, depths, poses, kw)
        got = _batch(ctx, depths, poses, kw)
    finally:
        assert L.i3d_debug_register_row_cap(ctx.h, 0) == 0
    for i in range(3):
        _same(got[i], one[i], f"frame {i} under the cap")
    assert one[0][1]["status"] == 0 and one[0][1]["valid_pixels"] == int((depth > 0).sum())
    assert not np.array_equal(one[0][0], free[0][0]) or one[0][1] != free[0][1]                     # another order of summation: the cap took effect
    uncapped = _batch(ctx, depths, poses, kw)
    for i in range(3):
        _same(uncapped[i], free[i], f"frame {i} without the cap")


def test_distortion_and_the_far_grid(contexts):
    """|t| is about 600 m here: a last-bit slip in the pivot or in the inversion of the pose would show"""
    ctx = contexts("shifted")
    key = ("shifted", "dist32", True, False)
    g, cam, depth, start, runs, _ = SC.checked_frame(key)
    assert np.abs(start[3:]).max() > 100.0 and np.abs(cam["dist"]).max() > 1e-5
    depths = np.stack([depth, depth]).astype(np.float32)
    poses = np.stack([start, np.asarray(cam["pose"], np.float64)])
    for desc in (dict(), dict(stride=2)):
        kw = _kw(cam, desc)
        one = _singles(ctx, depths, poses, kw)
        got = _batch(ctx, depths, poses, kw)
        for i in range(2):
            _same(got[i], one[i], f"{desc} frame {i}")
        assert one[0][1]["status"] == 0 and one[0][1]["iterations"] >= 2
    desc, tw_pose, tw = runs[0]
    ang, tr = ST.pose_err(_batch(ctx, depths, poses, _kw(cam, desc))[0][0], tw_pose, VS)
    b_ang, b_tr, _ = SC.order_bar(key, 0)
    quantum = SC.translation_quantum(tw_pose)
    print(f"far grid: against the twin {ang:.2e} rad {tr:.2e} voxel (bar {b_ang:.1e} / {b_tr:.1e}, one ulp of t {quantum:.1e} voxel)")
    assert ang <= b_ang
    if b_tr > 1e-12 or quantum < 1e-12:                     # track_sdf_cases.translation_quantum
        assert tr <= b_tr


def _keyframe_context():
    """the plain grid with three keyframes of two levels: the rendered 32 x 24 views from three poses and the 16 x 12 views of the halved camera"""
    g, cam, _, start, _, _ = SC.checked_frame(CLEAN)
    rng = np.random.default_rng(21)
    poses = np.stack([np.asarray(cam["pose"], np.float64), start, track_twin.perturb(cam["pose"], rng, 0.8, 1.5 * VS)])
    ctx = B.Context(0)
    ctx.set_grid(VS, g["keys"], g["sdf"], g["sdf_refined"], g["albedo"], g["weight"], g["color"])
    frames = []
    for p in poses:
        planes = []
        for level in (0, 1):
            w, h = cam["width"] >> level, cam["height"] >> level
            out = ctx.render_view(frame=-1, planes=("depth",), camera=dict(width=w, height=h, intr=np.asarray(cam["intr"]) / 2 ** level, dist=cam["dist"], pose=p))
            planes.append(np.ascontiguousarray(out["depth"], np.float32).reshape(h, w))
        frames.append(dict(lum=[np.full(d.shape, 0.5, np.float32) for d in planes], depth=planes))
    ctx.set_frames(frames, 2)
    ctx.set_camera(cam["intr"], cam["dist"], poses)
    return ctx, cam, poses


def test_keyframes():
    ctx, cam, kf_poses = _keyframe_context()
    try:
        rng = np.random.default_rng(22)
        starts = np.stack([track_twin.perturb(p, rng, 0.4, 0.8 * VS) for p in kf_poses])
        before = ctx.get_camera()
        for level in (0, 1):
            w, h = cam["width"] >> level, cam["height"] >> level
            images = [ctx.get_frame_image(f, level, w, h)[1] for f in range(3)]
            if level == 0:
                one = [ctx.track_frame_sdf(images[f], starts[f], use_context_camera=1) for f in range(3)]
                assert all(s["status"] == 0 and s["iterations"] >= 1 for _, s in one), [s for _, s in one]
            else:
                one = [ctx.track_frame_sdf(images[f], starts[f], intr=np.asarray(cam["intr"]) / 2, dist=cam["dist"]) for f in range(3)]
                assert all(s["valid_pixels"] == int((images[f] > 0).sum()) > 0 for f, (_, s) in enumerate(one))
            out, st = ctx.track_keyframes_sdf(starts, level=level)
            print(f"level {level}: " + "; ".join(f"status {s['status']} steps {s['iterations']} inliers {s['inliers']}" for s in st))
            for f in range(3):
                _same((out[f], st[f]), one[f], f"level {level} keyframe {f}")
            out, st = ctx.track_keyframes_sdf(starts[[2, 0]], level=level, frames=[2, 0])
            assert len(st) == 2
            _same((out[0], st[0]), one[2], f"level {level} frames=[2, 0] first")
            _same((out[1], st[1]), one[0], f"level {level} frames=[2, 0] second")
            out, st = ctx.track_keyframes_sdf(starts[[1, 1, 0]], level=level, frames=[1, 1, 0], stride=2)
            ref = [ctx.track_frame_sdf(images[f], starts[f], intr=np.asarray(cam["intr"]) / 2 ** level, dist=cam["dist"], stride=2) for f in (1, 1, 0)]
            for j in range(3):
                _same((out[j], st[j]), ref[j], f"level {level} repeated index, entry {j}")
        after = ctx.get_camera()
        for x, y in zip(before, after):
            assert x.tobytes() == y.tobytes()
        assert np.array_equal(after[2], kf_poses)           # the context's poses were neither read for the starts nor written
    finally:
        ctx.close()


SENTINEL = -12345.0


def test_errors_and_no_ops(contexts):
    L = B.load()
    p = B._p
    intr = [30.0, 30.0, 1.5, 1.5]
    D = lambda **kw: B.track_sdf_desc_default(intr=intr, **kw)
    d = D()
    dep = np.zeros((2, 4, 4), np.float32)
    good = np.full((2, 6), SENTINEL)                        # finite: where the pose is not the fault no earlier check hides the one under test
    zero = np.zeros((2, 6))

    def run(call, last_error, code, word, poses=None):
        """the call on sentinel-filled outputs: its code, a word of its message, and nothing written"""
        po = np.full((2, 6), SENTINEL) if poses is None else np.array(poses, np.float64)
        keep = po.copy()
        st = (B.TrackSdfStats * 2)()
        for s in st:
            s.iterations = s.status = -7; s.valid_pixels = s.valid = s.inliers = -7; s.rms_initial = s.rms_final = s.min_pivot_ratio = SENTINEL
        raw = bytes(st)
        rc = call(po, C.cast(st, C.c_void_p))
        assert rc == code, (word, rc, last_error())
        if word:
            assert word in last_error(), (word, last_error())
        assert po.tobytes() == keep.tobytes() and bytes(st) == raw, word

    ctx = contexts("plain")
    err = lambda: L.i3d_last_error(ctx.h).decode()
    frames = lambda dd, n, w, h, de: (lambda po, st: L.i3d_track_frames_sdf(ctx.h, dd, n, w, h, de, p(po), st))
    nan1 = good.copy(); nan1[1, 4] = np.nan
    inf0 = good.copy(); inf0[0, 0] = np.inf
    # I3D_ERR_INVALID_ARGUMENT
    run(lambda po, st: L.i3d_track_frames_sdf(None, d, 2, 4, 4, p(dep), p(po), st), lambda: "", 1, "", good)
    for call, word, poses in [(frames(None, 2, 4, 4, p(dep)), "descriptor", good), (frames(d, 2, 4, 4, None), "depth", good),
                              (lambda po, st: L.i3d_track_frames_sdf(ctx.h, d, 2, 4, 4, p(dep), None, st), "poses", good),
                              (frames(d, -1, 4, 4, p(dep)), "num_frames", good),
                              (frames(d, 2, 0, 4, p(dep)), "image size", good), (frames(d, 2, 4, -1, p(dep)), "image size", good),
                              (frames(d, 2, 32769, 4, p(dep)), "image size", good), (frames(d, 2, 4, 32769, p(dep)), "image size", good),
                              (frames(D(stride=0), 2, 4, 4, p(dep)), "stride", good), (frames(D(stride=17), 2, 4, 4, p(dep)), "stride", good),
                              (frames(D(iterations=-1), 2, 4, 4, p(dep)), "iterations", good), (frames(D(iterations=201), 2, 4, 4, p(dep)), "iterations", good),
                              (frames(D(max_distance=0.0), 2, 4, 4, p(dep)), "max_distance", good),
                              (frames(D(max_distance=float("nan")), 2, 4, 4, p(dep)), "max_distance", good),
                              (frames(D(max_distance=float("inf")), 2, 4, 4, p(dep)), "max_distance", good),
                              (frames(D(huber_delta=float("nan")), 2, 4, 4, p(dep)), "huber_delta", good),
                              (frames(D(huber_delta=float("inf")), 2, 4, 4, p(dep)), "huber_delta", good),
                              (frames(d, 2, 4, 4, p(dep)), "frame 1 is not finite", nan1), (frames(d, 2, 4, 4, p(dep)), "frame 0 is not finite", inf0),
                              (frames(B.track_sdf_desc_default(intr=[0.0, 30.0, 1.5, 1.5]), 2, 4, 4, p(dep)), "focal", good),
                              (frames(B.track_sdf_desc_default(intr=[30.0, -1.0, 1.5, 1.5]), 2, 4, 4, p(dep)), "focal", good)]:
        run(call, err, 1, word, poses)
    # I3D_ERR_STATE: no grid | the context's camera asked for without one
    with B.Context(0) as empty:
        e_err = lambda: L.i3d_last_error(empty.h).decode()
        run(lambda po, st: L.i3d_track_frames_sdf(empty.h, d, 2, 4, 4, p(dep), p(po), st), e_err, 4, "no grid", good)
        run(lambda po, st: L.i3d_track_keyframes_sdf(empty.h, D(use_context_camera=1), 0, 2, None, p(po), st), e_err, 4, "no grid", good)
    run(frames(D(use_context_camera=1), 2, 4, 4, p(dep)), err, 4, "camera", good)
    run(lambda po, st: L.i3d_track_keyframes_sdf(ctx.h, D(use_context_camera=1), 0, 2, None, p(po), st), err, 4, "no keyframes", good)
    # no-ops: zero frames return OK and touch nothing, whatever else is passed
    run(frames(d, 0, 4, 4, p(dep)), err, 0, "")
    run(lambda po, st: L.i3d_track_frames_sdf(ctx.h, d, 0, 4, 4, None, None, None), err, 0, "")
    run(lambda po, st: L.i3d_track_keyframes_sdf(ctx.h, D(use_context_camera=1), 0, 0, None, p(po), st), err, 0, "")
    out, st = ctx.track_frames_sdf(np.zeros((0, 4, 4), np.float32), np.zeros((0, 6)), intr=intr)
    assert out.shape == (0, 6) and st == []
    # a good call after all of it: stats may be null, and the statuses do not change the return code
    po = zero.copy()
    assert L.i3d_track_frames_sdf(ctx.h, D(iterations=200, stride=16), 2, 4, 4, p(dep), p(po), None) == 0 and np.array_equal(po, zero)
    with pytest.raises(B.I3DError) as e:
        ctx.track_frames_sdf(dep, zero, intr=intr, stride=99)
    assert "failed (1)" in str(e.value) and "stride" in str(e.value)
    assert L.i3d_debug_track_batch_frames(ctx.h, -3) == 0   # <= 0: the default rule


def test_keyframe_errors():
    L = B.load()
    p = B._p
    ctx, cam, kf_poses = _keyframe_context()
    try:
        err = lambda: L.i3d_last_error(ctx.h).decode()
        DC = lambda **kw: B.track_sdf_desc_default(use_context_camera=1, **kw)
        idx = lambda *a: p(np.array(a, np.int32))

        def run(call, code, word, poses=None):
            po = np.full((2, 6), SENTINEL) if poses is None else np.array(poses, np.float64)
            keep = po.copy()
            st = (B.TrackSdfStats * 3)()
            for s in st:
                s.status = -7; s.valid = -7; s.rms_final = SENTINEL
            raw = bytes(st)
            rc = call(po, C.cast(st, C.c_void_p))
            assert rc == code and word in err(), (word, rc, err())
            assert po.tobytes() == keep.tobytes() and bytes(st) == raw, word

        keys = lambda dd, level, n, fr: (lambda po, st: L.i3d_track_keyframes_sdf(ctx.h, dd, level, n, fr, p(po), st))
        nan1 = np.full((2, 6), SENTINEL); nan1[1, 2] = np.nan
        for call, word, poses in [(keys(None, 0, 2, idx(0, 1)), "descriptor", None), (keys(DC(), 0, -1, idx(0, 1)), "num", None),
                                  (lambda po, st: L.i3d_track_keyframes_sdf(ctx.h, DC(), 0, 2, idx(0, 1), None, st), "poses", None),
                                  (keys(B.track_sdf_desc_default(intr=cam["intr"]), 0, 2, idx(0, 1)), "use_context_camera", None),
                                  (keys(DC(), -1, 2, idx(0, 1)), "level", None), (keys(DC(), 2, 2, idx(0, 1)), "level", None),
                                  (keys(DC(), 0, 2, idx(0, 3)), "index 3", None), (keys(DC(), 0, 2, idx(-1, 0)), "index -1", None),
                                  (keys(DC(), 0, 2, None), "number of keyframes", None),
                                  (keys(DC(stride=17), 0, 2, idx(0, 1)), "stride", None), (keys(DC(max_distance=-1.0), 0, 2, idx(0, 1)), "max_distance", None),
                                  (keys(DC(), 0, 2, idx(0, 1)), "frame 1 is not finite", nan1)]:
            run(call, 1, word, poses)
        # I3D_ERR_STATE without a camera: the same keyframes on a context that was never given one
        g = RC.grid("plain")
        with B.Context(0) as bare:
            bare.set_grid(VS, g["keys"], g["sdf"], g["sdf_refined"], g["albedo"], g["weight"], g["color"])
            flat = [dict(lum=[np.full((24, 32), 0.5, np.float32)], depth=[np.ones((24, 32), np.float32)]) for _ in range(2)]
            bare.set_frames(flat, 1)
            po = np.zeros((2, 6))
            assert L.i3d_track_keyframes_sdf(bare.h, DC(), 0, 2, None, p(po), None) == 4 and "no camera" in L.i3d_last_error(bare.h).decode()
            assert not po.any()
        with pytest.raises(ValueError):
            ctx.track_keyframes_sdf(np.zeros((2, 6)), frames=[0])
    finally:
        ctx.close()


def test_a_batch_changes_nothing():
    """as test_gpu_track_sdf.test_tracking_on_the_field_changes_nothing: the grid export, the camera and one optimize step with and without batch calls in between"""
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
                depths, starts = np.stack([depth, depth]), np.stack([start, sc["truth"]])
                got = _batch(ctx, depths, starts, dict(use_context_camera=1, stride=2))
                assert got[0][1]["valid"] > 500 and got[0][1]["iterations"] >= 1
                one = _singles(ctx, depths, starts, dict(use_context_camera=1, stride=2))       # 160 x 120: 19 workgroups per frame
                for i in range(2):
                    _same(got[i], one[i], f"frame {i}")
                _, st = ctx.track_keyframes_sdf(sc["poses"], huber_delta=0.5 * vs)
                assert len(st) == 3 and all(s["valid_pixels"] > 0 for s in st)
            stats = ctx.optimize(cfg)
            if track:
                ctx.track_frames_sdf(depths, starts, intr=sc["intr"], refined=False, iterations=0)
                ctx.track_keyframes_sdf(np.asarray(sc["poses"])[[1]], frames=[1])
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
