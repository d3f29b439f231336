"""i3d_fusion_track_sdf_rgbd without a device: its symbols, the null handle, the numpy statement (fusion_track_sdf_rgbd_twin.py) against
central differences, the input conditions of the device tests (fusion_track_sdf_rgbd_cases.py) and the table of section 22.3 - what the fused colour pins that
depth cannot.  The oracle's Fusion supplies the volume.

Measured here, three starts 2 degrees about the sphere's centre and 1 voxel off, budget 60, library stop rule:
  96 x 72 (2220 depth pixels): depth only ends 13.56 / 7.92 / 6.59 degrees off (status 0 / 1 / 1); with the fused colour all three end 0.1995 degrees and 0.106
  voxel off, status 0 after 5 to 6 steps, 1825 samples = 1825 inliers, min_pivot_ratio 3.3e-4 .. 4.9e-4 against 0.9e-4 .. 1.6e-4.
  64 x 48 (988 depth pixels): depth only 10.19 / 11.80 / 4.45 degrees; with the colour 0.2668 degrees and 0.134 voxel, status 0 after 5 to 6 steps, 721 = 721.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fusion_track_sdf_rgbd_cases as FC
import fusion_track_sdf_rgbd_twin as FT
import track_sdf_rgbd_twin as PT
import track_sdf_twin as ST
import track_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("i3d_fusion_track_sdf_rgbd", "i3d_fusion_debug_voxel_luminance", "i3d_fusion_debug_track_sdf_rgbd_sums")


def test_symbols_are_declared_exported_and_typed():
    from intrinsic3d_amd import binding
    header = open(os.path.join(ROOT, "include", "intrinsic3d_hip.h")).read()
    for name in NAMES:
        assert name in binding.EXPORTS and re.search(r"\bint\s+" + name + r"\(i3d_fusion\* f,", header), name
    assert "There is no fusion variant" not in header
    L = binding.load()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert L.i3d_fusion_track_sdf_rgbd.restype is i32
    assert L.i3d_fusion_track_sdf_rgbd.argtypes == [vp, C.POINTER(binding.TrackSdfRgbdDesc), i32, i32, vp, vp, vp, C.POINTER(binding.TrackSdfRgbdStats)]
    assert L.i3d_fusion_debug_voxel_luminance.argtypes == [vp, i64, vp, vp]
    assert L.i3d_fusion_debug_track_sdf_rgbd_sums.argtypes == [vp, C.POINTER(binding.TrackSdfRgbdDesc), i32, i32, vp, vp, vp, vp, vp, C.POINTER(i64), C.POINTER(i64)]
    for m in ("track_sdf_rgbd", "debug_voxel_luminance", "debug_track_sdf_rgbd_sums"):
        assert callable(getattr(binding.Fusion, m))


def test_null_handle_is_an_invalid_argument():
    from intrinsic3d_amd import binding
    L = binding.load()
    p = binding._p
    d = binding.track_sdf_rgbd_desc_default(intr=[30.0, 30.0, 1.5, 1.5])
    dep = np.ones((4, 4), np.float32); lum = np.ones((4, 4), np.float32); pose = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6]); keep = pose.copy()
    st = binding.TrackSdfRgbdStats(); st.photo_samples = 7
    assert L.i3d_fusion_track_sdf_rgbd(None, d, 4, 4, p(dep), p(lum), p(pose), C.byref(st)) == 1
    assert st.photo_samples == 7 and np.array_equal(pose, keep)
    c = np.full(2, 5.0)
    assert L.i3d_fusion_debug_voxel_luminance(None, 2, p(np.zeros((2, 3), np.int32)), p(c)) == 1 and np.array_equal(c, [5.0, 5.0])
    s = np.full(31, -1.0)
    assert L.i3d_fusion_debug_track_sdf_rgbd_sums(None, d, 4, 4, p(dep), p(lum), p(pose), p(np.zeros(3)), p(s), None, None) == 1 and np.all(s == -1.0)


def test_luminance_volume_of_the_twin():
    """fp32 in k_lum_from_bgr's order on R, G, B; NaN where the weight is 0; a swapped channel gives another value"""
    ex = dict(weight=np.array([1.0, 0.0, 2.0], np.float32), color=np.array([[10, 200, 90], [1, 2, 3], [255, 255, 255]], np.uint8))
    c = FT.voxel_luminance(ex)
    s = np.float32(1.0 / 255.0)
    want = np.float32(np.float32(np.float32(np.float32(90) * s) * np.float32(0.114)) + np.float32(np.float32(np.float32(200) * s) * np.float32(0.587))) \
        + np.float32(np.float32(np.float32(10) * s) * np.float32(0.299))
    assert c[0] == float(np.float32(want)) and np.isnan(c[1]) and abs(c[2] - 1.0) < 1e-6
    assert FT.luminance(np.array([90, 200, 10], np.uint8)) != c[0]
    for w, h in FC.SIZES:
        for differ in (False, True):
            ex = FC.volume(w, h, differ)
            c = FT.voxel_luminance(ex)
            print(f"{w} x {h} differ {differ}: {c.size} voxels, c in [{np.nanmin(c):.3f}, {np.nanmax(c):.3f}], {int((c == 0.0).sum())} black")
            assert 2000 < c.size < 12000 and not np.isnan(c).any() and np.nanmax(c) > 0.4     # the export holds the voxels with weight != 0 only
    a, b = FC.volume(64, 48, False), FC.volume(64, 48, True)
    assert np.array_equal(a["keys"], b["keys"]) and np.array_equal(a["sdf"], b["sdf"]) and not np.array_equal(a["color"], b["color"])
    assert (b["color"][:, 0] != b["color"][:, 2]).mean() > 0.5 and (b["color"][:, 0] != b["color"][:, 1]).mean() > 0.5


def test_frame_luminance_lookup():
    """the colour pixel of a depth pixel: identity for one camera, NaN outside a smaller colour image, the integration's rounding for a larger one"""
    rng = np.random.default_rng(3)
    bgr = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    k = FC.intrinsics(64, 48).astype(np.float32)
    same = FT.frame_luminance(bgr, k, k, 64, 48)
    assert np.array_equal(same, FT.luminance(bgr[..., ::-1]).astype(np.float32))
    big = FT.frame_luminance(np.repeat(np.repeat(bgr, 2, 0), 2, 1), k, np.array([2 * k[0], 2 * k[1], 2 * k[2] + 0.5, 2 * k[3] + 0.5], np.float32), 64, 48)
    assert np.array_equal(big, same)
    small = FT.frame_luminance(bgr[:24, :32], k, k, 64, 48)
    assert np.isnan(small[24:, :]).all() and np.isnan(small[:, 32:]).all() and np.array_equal(small[:24, :32], same[:24, :32])


def test_photometric_row_matches_central_differences():
    """J_p against central differences of the twin's r_p under the left perturbation exp(delta) about the pivot, over the luminance volume"""
    for key in ((64, 48, 0), (96, 72, 1)):
        size, cam, depth, lum, start, runs, _ = FC.checked_frame(key)
        st = runs[1][2]
        grid, vol = FC.twin(*size)
        pts, lum_s, c = st["points"], st["lum"], st["pivot"]
        R, t = ST.pose_to_cw(start)
        tp = t - c
        J = PT.photo_rows(grid, vol, pts, R, tp, c)
        r0, cell0 = PT.photo_residual_at(grid, vol, pts, lum_s, R, tp, c)
        h = 1e-7
        worst, n = 0.0, 0
        for k in range(6):
            x = np.zeros(6); x[k] = h
            Rp, tpp = track_twin.apply_step(R, tp, x); Rm, tpm = track_twin.apply_step(R, tp, -x)
            rp, cp = PT.photo_residual_at(grid, vol, pts, lum_s, Rp, tpp, c); rm, cm = PT.photo_residual_at(grid, vol, pts, lum_s, Rm, tpm, c)
            same = np.isfinite(r0) & np.isfinite(rp) & np.isfinite(rm) & (cp == cell0).all(1) & (cm == cell0).all(1)
            num = (rp[same] - rm[same]) / (2.0 * h)
            scale = np.abs(J[same]).max()
            worst = max(worst, float(np.abs(num - J[same, k]).max() / scale)); n = max(n, int(same.sum()))
        print(f"{key}: {n} samples, worst |numeric - J_p| / max |J_p| = {worst:.2e}")
        assert n > 200 and worst < 1e-6


def test_without_photometric_term_the_twin_is_track_sdf_twin():
    for key in ((64, 48, 0), (64, 48, 1)):
        size, cam, depth, lum, start, runs, _ = FC.checked_frame(key)
        desc, pose, st = runs[0]
        grid, _ = FC.twin(*size)
        p2, s2 = ST.track(grid, depth, cam["intr"], cam["dist"], start, dict(iterations=desc["iterations"]), trace=True)
        assert np.array_equal(p2, pose)
        for k in ("iterations", "status", "valid_pixels", "valid", "inliers", "rms_initial", "rms_final", "min_pivot_ratio"):
            assert s2[k] == st[k], k
        assert st["photo_samples"] == 0 and st["photo_rms_final"] == 0.0


def test_frames_are_checked_and_every_branch_runs():
    """the input conditions of the device tests"""
    for key in FC.FRAMES:
        size, cam, depth, lum, start, runs, removed = FC.checked_frame(key)
        assert removed <= FC.MAX_REMOVED, (key, removed)
        for desc, pose, st in runs:
            d = FT.default_desc(**desc)
            a = st["trace"][0]
            if d["photo_weight"] > 0.0 and key[0] != "nan":
                assert a["samples"] == a["inliers"] or d["max_photo_residual"] > 0.0                # no normal, no axis neighbours: every inlier has a sample
            if key[0] == "nan":
                assert 0 < a["samples"] < a["inliers"]                                              # inliers whose pixel has no luminance
            if d["max_photo_residual"] > 0.0:
                formed = int(a["rp_mask"].sum())
                print(f"{key} {desc}: the photo gate keeps {a['samples']} of {formed}")
                assert 0.1 * formed < a["samples"] < 0.95 * formed
            if d["huber_delta"] > 0.0:
                assert (np.abs(a["r"][a["inlier_mask"]]) > d["huber_delta"]).sum() > 10
                assert (np.abs(a["r"][a["inlier_mask"]]) <= d["huber_delta"]).sum() > 10
    assert FC.checked_frame(("px1", 0, 0))[5][0][2]["trace"][0]["samples"] == 1
    assert FC.checked_frame(("row65", 0, 0))[5][0][2]["trace"][0]["samples"] > 20


@pytest.mark.parametrize("size", FC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_colour_pins_what_depth_cannot_twin(size):
    """the table of section 22.3: every depth-only run ends at >= 2 x the start's rotation error, every colour run with status 0 at <= 0.25 x"""
    w, h = size
    for k in range(3):
        _, cam, depth, lum, start, runs, _ = FC.checked_frame((w, h, k))
        (_, pose_d, st_d), (_, pose_c, st_c) = runs[:2]
        s_deg = track_twin.rot_err_deg(start, cam["pose"])
        d_deg = track_twin.rot_err_deg(pose_d, cam["pose"]); c_deg = track_twin.rot_err_deg(pose_c, cam["pose"])
        c_vox = track_twin.centre_err(pose_c, cam["pose"]) / FC.VS
        print(f"{w} x {h} ({st_d['valid_pixels']} depth pixels) start {k}: {s_deg:.3f} deg; depth only {d_deg:.4f} deg (status {st_d['status']}, {st_d['iterations']} steps, "
              f"ratio {st_d['min_pivot_ratio']:.2e}); colour {c_deg:.4f} deg {c_vox:.4f} voxel (status {st_c['status']}, {st_c['iterations']} steps, "
              f"{st_c['photo_samples']} samples of {st_c['inliers']} inliers, ratio {st_c['min_pivot_ratio']:.2e}); {d_deg / s_deg:.2f} x and {c_deg / s_deg:.3f} x the start")
        assert s_deg > 1.9
        assert d_deg >= 2.0 * s_deg
        assert st_c["status"] == 0 and c_deg <= 0.25 * s_deg
        assert st_c["photo_samples"] == st_c["inliers"] > 0
        if size == (64, 48):
            assert abs(c_deg - FC.TWIN_ERR_DEG_64[k]) <= 1e-3 * FC.TWIN_ERR_DEG_64[k], (c_deg, FC.TWIN_ERR_DEG_64[k])      # the recorded figure is the twin's


def test_order_bars():
    """100 x numpy-against-sequential, floor 1e-12: the bar of the device against the twin, per run with a budget"""
    for key in FC.FULL_FRAMES:
        for i, (desc, pose, st) in enumerate(FC.checked_frame(key)[5]):
            if FT.default_desc(**desc)["iterations"] == 0:
                continue
            b_ang, b_tr, (ang, tr) = FC.order_bar(key, i)
            print(f"{key} run {i} ({st['iterations']} steps): numpy against sequential {ang:.2e} rad {tr:.2e} voxel")
            assert b_ang >= 1e-12 and b_tr >= 1e-12
