"""i3d_fusion_track_sdf_rgbd on the device, through the C ABI: the luminance volume and one pass of the combined sums against the numpy
statement (fusion_track_sdf_rgbd_twin.py) on the checked frames of fusion_track_sdf_rgbd_cases.py, the registration against the twin, the sphere that depth cannot
pin, the reduction to i3d_fusion_track_sdf, what the calls must leave alone, the errors and app_fusion's track_mode "sdf_rgbd"."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fusion_track_sdf_rgbd_cases as FC
import fusion_track_sdf_rgbd_twin as FT
import helpers
import track_sdf_twin as ST
import track_twin
from intrinsic3d_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

VS = FC.VS
INT_STATS = ("iterations", "status", "valid_pixels", "valid", "inliers", "photo_samples")
CAPACITY = 1 << 16


def _volume(w, h, colour=None, initial_capacity=CAPACITY, frames=None):
    return FC.fuse(B.Fusion(VS, 0.1, 10.0, initial_capacity=initial_capacity), w, h, frames=frames, colour=colour)


def _same_export(a, b):
    for k in ("keys", "sdf", "weight", "color"):
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def volumes():
    """one device volume per image size, the four frames fused and not finished, created on first use; its table is the oracle's (checked on a copy)"""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = _volume(w, h)
            with _volume(w, h) as copy:
                copy.finish(0)
                _same_export(copy.export(), FC.volume(w, h))
        return made[(w, h)]
    yield get
    for f in made.values():
        f.close()


# ---- 1. the luminance volume ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [CAPACITY, 1 << 10], ids=["roomy", "grown"])
def test_luminance_volume_equals_twin_bit_for_bit(capacity):
    """fp32 arithmetic in a fixed order: the same bits and the same NaN pattern.  The channels of the fused frames differ, so a swapped channel fails.  Queried:
    every allocated voxel (those with weight 0 are stored and have no luminance), keys that are not stored, keys that cannot be packed"""
    w, h = 64, 48
    raw = FC.raw_volume(w, h, True)
    tw = FT.voxel_luminance(raw)
    zero = raw["weight"] == 0.0
    rng = np.random.default_rng(5)
    absent = np.concatenate([raw["keys"][:50] + 1000, rng.integers(-5000, 5000, (50, 3)) + 20000, [[1 << 20, 0, 0], [0, -(1 << 20) - 1, 0], [0, 0, 2 ** 31 - 1]]]).astype(np.int32)
    with _volume(w, h, colour=FC.channels, initial_capacity=capacity) as f:
        for stage in ("fusing", "finished"):
            dev = f.debug_voxel_luminance(raw["keys"])
            assert np.array_equal(np.isnan(dev), zero) and zero.sum() > 100 and (~zero).sum() > 2000
            assert np.array_equal(dev[~zero].view(np.uint64), tw[~zero].view(np.uint64)), stage
            assert np.isnan(f.debug_voxel_luminance(absent)).all()
            if stage == "fusing":
                f.finish(0)
        _same_export(f.export(), FC.volume(w, h, True))
        info = f.info()
        print(f"capacity {info['capacity']} slots, {info['allocated']} allocated, {int((~zero).sum())} with a luminance in [{np.nanmin(dev):.3f}, {np.nanmax(dev):.3f}]")
        assert info["allocated"] == raw["keys"].shape[0] and (info["capacity"] > 4096 if capacity < CAPACITY else info["capacity"] == 2 * CAPACITY)
    swapped = FT.luminance(raw["color"][~zero][:, ::-1])
    assert (swapped != tw[~zero]).mean() > 0.9


# ---- 2. one pass of the sums ---------------------------------------------------------------------------------------------------------------------------------
def _check_sums(dev, valid, samples, tw, n, what):
    assert valid == tw["valid"] and int(dev[28]) == tw["inliers"] and samples == tw["samples"] == int(dev[30]), (what, valid, tw["valid"], dev[28], tw["inliers"],
                                                                                                                  samples, tw["samples"], dev[30])
    err = np.abs(dev - tw["sums"]); tol = n * 2.0 ** -52 * tw["abs_sums"]
    print(f"  {what}: n = {n}, valid {valid}, inliers {tw['inliers']}, photometric samples {samples}, worst error / bound {np.max(err / np.maximum(tol, 1e-300)):.3f}")
    assert np.all(err <= tol), (what, err, tol)


SUM_FRAMES = [(64, 48, 0), (96, 72, 1), ("px1", 0, 0), ("row65", 0, 0), ("nan", 0, 0)]


@pytest.mark.parametrize("key", SUM_FRAMES, ids=lambda k: "-".join(str(x) for x in k))
def test_sums_equal_twin(volumes, key):
    """strides 1, 2 and 3, Huber on and off, a photo gate that cuts a part, geometric_weight = 0, a 1 x 1 and a 65 x 1 image (tail lanes), a frame with NaN
    luminance pixels; the same call twice gives the same bits"""
    size, cam, depth, lum, start, runs, _ = FC.checked_frame(key)
    f = volumes(*size)
    for i, (desc, _, st) in enumerate(runs):
        tw, c = FC.twin_start_sums(key, i)
        n = st["points"].shape[0]
        dev, valid, samples = f.debug_track_sdf_rgbd_sums(depth, lum, start, c, cam["intr"], **desc)
        _check_sums(dev, valid, samples, tw, n, f"{key} {desc}")
        again = f.debug_track_sdf_rgbd_sums(depth, lum, start, c, cam["intr"], **desc)
        assert np.array_equal(dev, again[0]) and (valid, samples) == again[1:]
        if desc.get("photo_weight", 0.1) == 0.0:
            assert samples == 0 and dev[29] == 0.0
        if desc.get("max_photo_residual", 0.0) > 0.0:
            assert 0 < tw["samples"] < int(tw["rp_mask"].sum())
        if key[0] == "nan":
            assert 0 < tw["samples"] < tw["inliers"]
        if desc.get("geometric_weight", 1.0) == 0.0:
            plain, _ = FC.twin_start_sums(key, 1)
            assert tw["samples"] == plain["samples"] and not np.array_equal(tw["sums"][:27], plain["sums"][:27]) and tw["sums"][27] == plain["sums"][27]


# ---- 3. full runs --------------------------------------------------------------------------------------------------------------------------------------------
def _check_against_twin(key, i, pose, st, tw_pose, tw):
    b_ang, b_tr, _ = FC.order_bar(key, i)
    ang, tr = ST.pose_err(pose, tw_pose, VS)
    print(f"{key} run {i}: status {st['status']} steps {st['iterations']} (twin {tw['status']} / {tw['iterations']}); against the twin {ang:.2e} rad {tr:.2e} voxel "
          f"(bar {b_ang:.1e} / {b_tr:.1e}); rms {st['rms_initial']:.3e} -> {st['rms_final']:.3e}; photo rms {st['photo_rms_initial']:.3e} -> "
          f"{st['photo_rms_final']:.3e} on {st['photo_samples']} of {st['inliers']}; ratio {st['min_pivot_ratio']:.3e}")
    assert all(st[k] == tw[k] for k in INT_STATS), (st, {k: tw[k] for k in INT_STATS})
    assert ang <= b_ang and tr <= b_tr
    for k in ("rms_initial", "photo_rms_initial"):
        assert abs(st[k] - tw[k]) <= 1e-12 * tw[k], k
    for k in ("rms_final", "photo_rms_final", "min_pivot_ratio"):
        assert abs(st[k] - tw[k]) <= 1e-6 * tw[k], k


@pytest.mark.parametrize("key", FC.FULL_FRAMES, ids=lambda k: "-".join(str(x) for x in k))
def test_registration_equals_twin(volumes, key):
    size, cam, depth, lum, start, runs, _ = FC.checked_frame(key)
    f = volumes(*size)
    for i in (0, 1):
        desc, tw_pose, tw = runs[i]
        pose, st = f.track_sdf_rgbd(depth, lum, start, cam["intr"], **desc)
        _check_against_twin(key, i, pose, st, tw_pose, tw)
        pose_b, st_b = f.track_sdf_rgbd(depth, lum, start, cam["intr"], **desc)
        assert np.array_equal(pose, pose_b) and st == st_b                                          # the same input gives the same bits


# ---- 4. colour pins what depth cannot ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_colour_pins_what_depth_cannot(volumes, k):
    """the CPU test's two assertions on the device's poses at 64 x 48, and the device's error against the truth within DEVICE_TWIN_BAR x the twin's recorded one"""
    key = (64, 48, k)
    size, cam, depth, lum, start, runs, _ = FC.checked_frame(key)
    f = volumes(*size)
    s_deg = track_twin.rot_err_deg(start, cam["pose"])
    pose_d, st_d = f.track_sdf_rgbd(depth, lum, start, cam["intr"], **runs[0][0])
    pose_c, st_c = f.track_sdf_rgbd(depth, lum, start, cam["intr"], **runs[1][0])
    d_deg, c_deg = track_twin.rot_err_deg(pose_d, cam["pose"]), track_twin.rot_err_deg(pose_c, cam["pose"])
    print(f"start {k}: {s_deg:.3f} deg; depth only {d_deg:.4f} deg (status {st_d['status']}); colour {c_deg:.6f} deg (status {st_c['status']}, {st_c['iterations']} steps); "
          f"device / twin {c_deg / FC.TWIN_ERR_DEG_64[k]:.6f}")
    assert d_deg >= 2.0 * s_deg and st_d["photo_samples"] == 0
    assert st_c["status"] == 0 and c_deg <= 0.25 * s_deg
    assert c_deg <= FC.DEVICE_TWIN_BAR * FC.TWIN_ERR_DEG_64[k]
    assert st_c["min_pivot_ratio"] > st_d["min_pivot_ratio"]


# ---- 5. the reduction ----------------------------------------------------------------------------------------------------------------------------------------
def test_without_photo_weight_it_is_fusion_track_sdf_byte_for_byte(volumes):
    size, cam, depth, lum, start, _, _ = FC.checked_frame((64, 48, 0))
    f = volumes(*size)
    for desc in (dict(), dict(stride=2), dict(stride=3, iterations=2), dict(huber_delta=FC.HUBER), dict(stride=2, huber_delta=FC.HUBER, iterations=0)):
        a_pose, a = f.track_sdf(depth, start, cam["intr"], **desc)
        b_pose, b = f.track_sdf_rgbd(depth, lum, start, cam["intr"], photo_weight=0.0, geometric_weight=1.0, **desc)
        assert a_pose.tobytes() == b_pose.tobytes(), desc
        for k in a:
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (desc, k, a[k], b[k])
        assert (b["photo_samples"], b["photo_rms_initial"], b["photo_rms_final"]) == (0, 0.0, 0.0)
        assert a["inliers"] > 64


# ---- 6. state ------------------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b, what):
    assert a[0].tobytes() == b[0].tobytes(), (what, a[0], b[0])
    for k in a[1]:
        assert np.float64(a[1][k]).tobytes() == np.float64(b[1][k]).tobytes(), (what, k, a[1][k], b[1][k])


def test_calls_change_nothing_and_see_the_table_as_it_stands(tmp_path):
    w, h = 64, 48
    size, cam, depth, lum, start, _, _ = FC.checked_frame((w, h, 0))
    intr = cam["intr"]
    i32 = intr.astype(np.float32)
    call = lambda f, **kw: f.track_sdf_rgbd(depth, lum, start, intr, **kw)  # noqa: E731
    frames = FC.fused_frames(w, h)
    keys = FC.raw_volume(w, h)["keys"]
    # integrate, finish, export and save with calls in between against the same without
    out = []
    for calls in (False, True):
        with B.Fusion(VS, 0.1, 10.0, initial_capacity=1 << 10) as f:
            if calls:
                st0 = call(f)                                                                       # before the first integrate: nothing to register on
                assert st0[1]["status"] == 2 and st0[0].tobytes() == np.asarray(start, np.float64).tobytes() and st0[1]["valid"] == 0
            for d, bgr, p in frames:
                f.integrate(d, i32, bgr, i32, FC.c2w(p), 2)
                if calls:
                    call(f, iterations=2); f.debug_voxel_luminance(keys[:100]); f.debug_track_sdf_rgbd_sums(depth, lum, start, np.zeros(3), intr, stride=2)
            n = f.finish(10)
            if calls:
                call(f, huber_delta=FC.HUBER)
            ex = f.export()
            f.save(tmp_path / f"vol{int(calls)}.tsdf")
            out.append((n, ex))
    assert out[0][0] == out[1][0]
    _same_export(out[0][1], out[1][1])
    assert open(tmp_path / "vol0.tsdf", "rb").read() == open(tmp_path / "vol1.tsdf", "rb").read()
    # no stale volume: the call after one more integrate is a fresh volume's call after the same five frames; finish(0) changes nothing
    _, d5, _, truth = FC.tracked_frame(w, h)
    bgr5 = np.full((h, w, 3), 200, np.uint8)
    five = list(frames) + [(d5, bgr5, truth)]
    with _volume(w, h, initial_capacity=1 << 10) as f, _volume(w, h, frames=five) as fresh:
        first = call(f)
        f.integrate(d5, i32, bgr5, i32, FC.c2w(truth), 2)
        moved = call(f)
        _same(moved, call(fresh), "after one more integrate")
        assert moved[1]["photo_rms_initial"] != first[1]["photo_rms_initial"] and moved[0].tobytes() != first[0].tobytes()
        f.finish(0)
        _same(call(f), moved, "after finish(0)")


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------------------------------
def test_errors(volumes):
    L = B.load()
    p = B._p
    dep = np.zeros((4, 4), np.float32); lum = np.zeros((4, 4), np.float32); pose = np.zeros(6)
    intr = [30.0, 30.0, 1.5, 1.5]
    D = lambda **kw: B.track_sdf_rgbd_desc_default(intr=intr, **kw)  # noqa: E731
    d = D()
    f = volumes(64, 48)
    msg = lambda: L.i3d_fusion_last_error(f.h).decode()  # noqa: E731
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
             ((D(max_photo_residual=nan), 4, 4, p(dep), p(lum), p(pose), None), "max_photo_residual"), ((D(max_photo_residual=inf), 4, 4, p(dep), p(lum), p(pose), None), "max_photo_residual"),
             ((D(use_context_camera=1), 4, 4, p(dep), p(lum), p(pose), None), "use_context_camera")]
    for args, word in cases:
        st = B.TrackSdfRgbdStats(); st.photo_samples = 7; st.base.valid = 9
        po = args[5]
        keep = None if po is None else np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_double)), (6,)).copy()
        a = args[:6] + (C.byref(st),)
        assert L.i3d_fusion_track_sdf_rgbd(f.h, *a) == 1 and word in msg(), (word, msg())
        assert st.photo_samples == 7 and st.base.valid == 9                                         # the outputs untouched
        if keep is not None:
            assert np.array_equal(np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_double)), (6,)), keep, equal_nan=True)
    # a frame without data: status 2, the figures zero; stats may be null
    st = B.TrackSdfRgbdStats(); st.base.valid = 7; st.photo_rms_final = 3.0
    assert L.i3d_fusion_track_sdf_rgbd(f.h, D(iterations=200, stride=16), 4, 4, p(dep), p(lum), p(pose), C.byref(st)) == 0
    assert st.base.status == 2 and st.base.valid == 0 and st.photo_rms_final == 0.0
    assert L.i3d_fusion_track_sdf_rgbd(f.h, d, 4, 4, p(dep), p(lum), p(pose), None) == 0
    s = np.full(31, -1.0)
    assert L.i3d_fusion_debug_track_sdf_rgbd_sums(f.h, d, 4, 4, p(dep), p(lum), None, p(pose[:3].copy()), p(s), None, None) == 1 and np.all(s == -1.0)
    assert L.i3d_fusion_debug_track_sdf_rgbd_sums(f.h, D(use_context_camera=1), 4, 4, p(dep), p(lum), p(pose), p(pose[:3].copy()), p(s), None, None) == 1
    assert L.i3d_fusion_debug_voxel_luminance(f.h, 2, None, p(np.zeros(2))) == 1 and L.i3d_fusion_debug_voxel_luminance(f.h, -1, None, None) == 1
    assert L.i3d_fusion_debug_voxel_luminance(f.h, 0, None, None) == 0
    with pytest.raises(B.I3DError) as e:
        f.track_sdf_rgbd(dep, lum, pose, intr, photo_weight=-1.0)
    assert "failed (1)" in str(e.value) and "weights" in str(e.value)
    # geometric_weight = 0: status 2 goes by the photometric samples (fewer than 64 here although the inliers are many)
    size, cam, depth, lum64, start, _, _ = FC.checked_frame((64, 48, 0))
    pose_g, st_g = f.track_sdf_rgbd(depth, lum64, start, cam["intr"], geometric_weight=0.0, max_photo_residual=0.002)
    assert st_g["status"] == 2 and st_g["inliers"] > 64 > st_g["photo_samples"] and np.array_equal(pose_g, start)


# ---- 8. app_fusion -------------------------------------------------------------------------------------------------------------------------------------------
def test_app_fusion_track_mode_sdf_rgbd(tmp_path):
    import make_dataset
    app = os.path.join(ROOT, "apps", "app_fusion")
    assert os.path.exists(app), "apps/app_fusion has not been built (run __graft_entry__.build())"
    w, h = 64, 48
    frames = FC.fused_frames(w, h)
    sc = dict(voxel_size=VS, intr=FC.intrinsics(w, h), keys=np.zeros((1, 3), np.int32), sdf=np.zeros(1, np.float32), weight=np.ones(1, np.float32),
              color=np.zeros((1, 3), np.uint8), frames=[dict(depth=[d], bgr=[bgr]) for d, bgr, _ in frames], poses=[p for _, _, p in frames])
    runs = {}
    for name, extra in (("plain", ""), ("off", 'track_frames: "0"\ntrack_mode: "sdf_rgbd"\ntrack_photo_weight: "0.2"\n'),
                        ("tracked", 'track_frames: "1"\ntrack_mode: "sdf_rgbd"\ntrack_photo_weight: "0.2"\noutput_tracked_poses: "./fusion/tracked.txt"\n')):
        out = tmp_path / name
        s, _ = make_dataset.write_dataset(str(out), sc)
        with open(out / "fusion.yml", "a") as fh:
            fh.write(extra)
        r = subprocess.run([app, "-s", s, "-f", str(out / "fusion.yml")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[name] = (out, r.stdout)
    tsdf = f"volume_{VS:g}.tsdf"
    read = lambda name: open(runs[name][0] / "fusion" / tsdf, "rb").read()  # noqa: E731
    assert read("plain") == read("off") and "tracking frame" not in runs["off"][1]
    text = runs["tracked"][1]
    assert text.count("tracking frame") == len(frames) - 1 and text.count("photometric:") == len(frames) - 1, text
    samples = [int(ln.split()[1]) for ln in text.splitlines() if ln.strip().startswith("photometric:")]
    assert all(n > 300 for n in samples), samples
    traj = helpers.read_tum(runs["tracked"][0] / "fusion" / "tracked.txt")
    assert traj.shape == (len(frames), 8)
    assert len(B.tsdf_read(str(runs["tracked"][0] / "fusion" / tsdf))["sdf"]) > 2000
