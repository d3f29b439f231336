"""i3d_track_frame_sdf_rgbd without a device: the ctypes mirrors of its structs and its defaults, the numpy statement (track_sdf_rgbd_twin.py) against central
differences and against track_sdf_twin, the input conditions of the device tests (track_sdf_rgbd_cases.py) and where the recorded bars come from.

Measured here.
  The shells (32 x 24, 136 to 548 usable samples, 47 % of the inliers with a photometric sample): the runs of TRUTH_RUNS end 1.0e-4 to 4.4e-4 rad and 3.1e-3 to
  1.3e-2 voxel from the render pose, status 0 after 4 to 6 steps - except `shifted` and `negative` at the plain camera with the refined field, which run their
  budget of 30 and end with status 1 at the same error (3.0e-4 rad, 5.3e-3 voxel): the limit cycle of section 21.3.
  The smooth sphere (80 x 60, 1572 usable samples, 1217 to 1431 inliers of which 770 to 1043 have a photometric sample; starts 2 degrees about the centre and 2.4
  to 4.1 voxels off; stop 1e-6, budget 60): depth only ends 10.4 to 12.0 degrees / 8.8 to 10.1 voxels off (status 1 after 60 steps twice, status 0 after 38 once);
  with photo_weight 0.1 all three starts end at one pose, 3.67e-4 rad (0.021 degrees) / 1.85e-2 voxel off, status 0 after 5 to 6 steps, min_pivot_ratio 3e-6 ..
  1.5e-5 -> 3e-4 .. 1.1e-3.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import track_sdf_cases as SC
import track_sdf_rgbd_cases as PC
import track_sdf_rgbd_twin as PT
import track_sdf_twin as ST
import track_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_and_defaults():
    from intrinsic3d_amd import binding
    fields = {"i3d_track_sdf_rgbd_desc": binding.TrackSdfRgbdDesc, "i3d_track_sdf_rgbd_stats": binding.TrackSdfRgbdStats}
    body = "".join(f'printf("%zu\\n", sizeof({n}));' for n in fields)
    for n, cls in fields.items():
        body += "".join(f'printf("%zu\\n", offsetof({n}, {f}));' for f, _ in cls._fields_)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "intrinsic3d_hip.h"\nint main(){' + body + 'return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    want = [ctypes.sizeof(c) for c in fields.values()]
    for cls in fields.values():
        want += [getattr(cls, f).offset for f, _ in cls._fields_]
    assert got == want
    for name in ("i3d_track_sdf_rgbd_desc_default", "i3d_track_frame_sdf_rgbd", "i3d_track_frames_sdf_rgbd", "i3d_track_keyframes_sdf_rgbd",
                 "i3d_debug_track_sdf_rgbd_sums", "i3d_debug_voxel_intensity"):
        assert name in binding.EXPORTS
    d = binding.track_sdf_rgbd_desc_default()
    assert bytes(d.base) == bytes(binding.track_sdf_desc_default())
    assert (d.geometric_weight, d.photo_weight, d.max_photo_residual, d.pad) == (1.0, 0.1, 0.0, 0)
    d = binding.track_sdf_rgbd_desc_default(photo_weight=0.25, stride=2, refined=False)
    assert d.photo_weight == 0.25 and d.base.stride == 2 and d.base.use_refined_sdf == 0 and d.base.iterations == 30
    tw = PT.default_desc()
    assert (tw["geometric_weight"], tw["photo_weight"], tw["max_photo_residual"]) == (1.0, 0.1, 0.0)


def test_intensity_volume_has_defined_and_undefined_voxels():
    for name in ("plain", "smooth"):
        g = PC.twin_grid(name)
        c, mag = PT.voxel_intensity(g, with_terms=True)
        nan = np.isnan(c)
        print(f"{name}: {c.size} voxels, {int(nan.sum())} without an intensity; c in [{np.nanmin(c):.3f}, {np.nanmax(c):.3f}]")
        assert 0 < nan.sum() < c.size and np.all(np.abs(c[~nan]) <= mag[~nan] * (1.0 + 1e-12))
        assert nan[g.weight == 0.0].all()
    # the weight-0 voxel of the shell and its six neighbours have none; the rim of the band has none
    g = PC.twin_grid("plain")
    hole = np.nonzero(g.weight == 0.0)[0]
    assert hole.size == 1
    nb = [g.find(g.keys[hole] + PT.AXIS[i])[0] for i in range(6)]
    assert all(n >= 0 for n in nb) and np.isnan(PT.voxel_intensity(g)[nb]).all()


def test_photometric_row_matches_central_differences():
    """J_p against central differences of the twin's r_p under the left perturbation exp(delta) about the pivot"""
    for key in (("plain", "plain32", True, 0), ("smooth", "level1", True, 0)):
        cam, depth, lum, start, runs, _ = PC.checked_frame(key)
        st = runs[-1][2]
        grid = PC.twin_grid(key[0], key[2])
        vol, pts, lum_s, c = st["vol"], st["points"], st["lum"], st["pivot"]
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


@pytest.mark.parametrize("key", [("plain", "plain32", True, False), ("shifted", "dist32", True, False), ("negative", "plain32", False, False),
                                 ("plain", "plain32", True, True)], ids=lambda k: "-".join(str(x) for x in k))
def test_without_photometric_term_the_twin_is_track_sdf_twin(key):
    g, cam, depth, start, runs, _ = SC.checked_frame(key)
    grid = SC.Q.twin_grid(g, key[2])
    lum = np.full(depth.shape, 0.5, np.float32)
    for desc, pose, st in runs:
        p2, s2 = PT.track(grid, depth, lum, cam["intr"], cam["dist"], start, dict(desc, photo_weight=0.0, geometric_weight=1.0), trace=True)
        assert np.array_equal(p2, pose)
        for k in ("iterations", "status", "valid_pixels", "valid", "inliers", "rms_initial", "rms_final", "min_pivot_ratio"):
            assert s2[k] == st[k], k
        assert s2["photo_samples"] == 0 and s2["photo_rms_final"] == 0.0
        assert all(np.array_equal(a["sums"][:29], b["sums"]) for a, b in zip(s2["trace"], st["trace"]))


def test_frames_are_checked_and_both_branches_run():
    """the input conditions of the device tests: the check removes at most MAX_REMOVED, inliers without a photometric sample exist, the photo gate cuts a part"""
    for key in PC.FRAMES:
        cam, depth, lum, start, runs, removed = PC.checked_frame(key)
        assert removed <= PC.MAX_REMOVED, (key, removed)
        for desc, pose, st in runs:
            d = PT.default_desc(**desc)
            a = st["trace"][0]
            if d["photo_weight"] > 0.0 and a["inliers"] >= 8:
                assert 0 < a["samples"] < a["inliers"], (key, desc, a["samples"], a["inliers"])
            if d["max_photo_residual"] > 0.0:
                formed = int(a["rp_mask"].sum())
                print(f"{key}: the photo gate keeps {a['samples']} of {formed}")
                assert 0.1 * formed < a["samples"] < 0.9 * formed
            if d["huber_delta"] > 0.0 and key[1] != "plain64":
                assert (np.abs(a["r"][a["inlier_mask"]]) > d["huber_delta"]).sum() > 10


def test_shell_runs_and_where_the_truth_bar_comes_from():
    worst = [0.0, 0.0]
    for key, i in PC.TRUTH_RUNS:
        cam, depth, lum, start, runs, _ = PC.checked_frame(key)
        desc, pose, st = runs[i]
        ang, tr = ST.pose_err(pose, cam["pose"], PC.VS)
        s_ang, s_tr = ST.pose_err(start, cam["pose"], PC.VS)
        print(f"{key} run {i}: status {st['status']} after {st['iterations']} steps; {s_ang:.3e} rad {s_tr:.3e} voxel -> {ang:.3e} rad {tr:.3e} voxel; "
              f"photo rms {st['photo_rms_initial']:.3e} -> {st['photo_rms_final']:.3e}, {st['photo_samples']} of {st['inliers']} inliers")
        # the limit cycle (section 21.3): a run may use its budget; it still ends at the pose of the converged ones
        assert st["status"] in (0, 1) and (st["status"] == 0 or st["iterations"] == 30)
        assert ang < 0.1 * s_ang and tr < 0.1 * s_tr and st["photo_rms_final"] < 0.5 * st["photo_rms_initial"]
        worst = [max(worst[0], ang), max(worst[1], tr)]
    print(f"the twin against the render pose: <= {worst[0]:.3e} rad, {worst[1]:.3e} voxel; bars {PC.TRUTH_BAR_RAD} / {PC.TRUTH_BAR_VOX}")
    assert 2.0 * worst[0] <= PC.TRUTH_BAR_RAD <= 2.5 * worst[0] and 2.0 * worst[1] <= PC.TRUTH_BAR_VOX <= 2.5 * worst[1]


def test_colour_pins_what_depth_cannot_twin():
    """the smooth sphere: depth only ends no closer in rotation than it started; with the photometric term all three starts converge, to one pose"""
    vs = PC.model("smooth")["voxel_size"]
    ends, worst = [], [0.0, 0.0]
    for key in PC.SMOOTH_FRAMES:
        cam, depth, lum, start, runs, _ = PC.checked_frame(key)
        (_, pose_d, st_d), (_, pose_c, st_c) = runs
        s_ang, s_tr = ST.pose_err(start, cam["pose"], vs)
        d_ang, d_tr = ST.pose_err(pose_d, cam["pose"], vs)
        c_ang, c_tr = ST.pose_err(pose_c, cam["pose"], vs)
        print(f"start {np.degrees(s_ang):.3f} deg {s_tr:.2f} voxel: depth only {np.degrees(d_ang):.3f} deg {d_tr:.2f} voxel (status {st_d['status']}, {st_d['iterations']} "
              f"steps); rgbd {c_ang:.3e} rad ({np.degrees(c_ang):.4f} deg) {c_tr:.3e} voxel (status {st_c['status']}, {st_c['iterations']} steps, "
              f"{st_c['photo_samples']} of {st_c['inliers']} inliers), min_pivot_ratio {st_d['min_pivot_ratio']:.2e} -> {st_c['min_pivot_ratio']:.2e}")
        assert np.degrees(s_ang) > 1.9 and d_ang >= s_ang
        assert st_c["status"] == 0 and st_c["iterations"] <= 10 and c_ang < 0.05 * s_ang and c_tr < 0.05 * s_tr
        assert st_c["min_pivot_ratio"] > 10.0 * st_d["min_pivot_ratio"] and st_c["photo_rms_final"] < 0.25 * st_c["photo_rms_initial"]
        ends.append(pose_c); worst = [max(worst[0], c_ang), max(worst[1], c_tr)]
    for p in ends[1:]:
        ang, tr = ST.pose_err(p, ends[0], vs)
        assert ang < 1e-5 and tr < 1e-3, (ang, tr)
    print(f"the twin against the truth: <= {worst[0]:.3e} rad, {worst[1]:.3e} voxel; bars {PC.SMOOTH_BAR_RAD} / {PC.SMOOTH_BAR_VOX}")
    assert 2.0 * worst[0] <= PC.SMOOTH_BAR_RAD <= 2.5 * worst[0] and 2.0 * worst[1] <= PC.SMOOTH_BAR_VOX <= 2.5 * worst[1]


def test_order_bars():
    """100 x numpy-against-sequential, floor 1e-12: the bar of the device against the twin, per run with a budget"""
    for key in PC.FRAMES:
        for i, (desc, pose, st) in enumerate(PC.checked_frame(key)[4]):
            if PT.default_desc(**desc)["iterations"] == 0:
                continue
            b_ang, b_tr, (ang, tr) = PC.order_bar(key, i)
            print(f"{key} run {i} ({st['iterations']} steps): numpy against sequential {ang:.2e} rad {tr:.2e} voxel; one ulp of t {PC.translation_quantum(pose):.1e} voxel")
            assert b_ang >= 1e-12 and b_tr >= 1e-12
