"""-m "not gpu": the numpy statement of i3d_track_frame_sdf (track_sdf_twin.py) on the checked frames of track_sdf_cases.py - the input conditions the device
comparison relies on, the bars it is held to - and what the entry points do without a device: struct layouts, symbols, defaults, argument errors."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import query_cases as Q
import register_twin as RT
import track_sdf_cases as SC
import track_sdf_twin as ST
import track_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VS = SC.VS


def _lib():
    from intrinsic3d_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return binding, binding.load()


@pytest.mark.parametrize("key", list(SC.FRAMES), ids=lambda k: "-".join(str(x) for x in k))
def test_checked_frames_meet_the_input_conditions(key):
    g, cam, depth, start, runs, removed = SC.checked_frame(key)
    grid = Q.twin_grid(g, key[2])
    usable = int((depth > 0).sum())
    print(f"{key}: {usable} usable pixels, share removed by the check {removed:.4f}")
    assert removed <= SC.MAX_REMOVED and usable >= 1
    for desc, pose, st in runs:
        again, st2 = ST.track(grid, depth, cam["intr"], cam["dist"], start, desc, trace=True)       # the frame as the device test will see it
        assert np.array_equal(again, pose)
        face, gate = SC.run_margins(grid, st2, desc)
        assert face.min() >= SC.FACE_MARGIN and gate.min() >= SC.GATE_MARGIN
        d = ST.default_desc(**desc)
        for nw, nu in st2["steps"]:                                                                 # no step sits on the stop rule
            assert abs(nw / d["stop_rotation"] - 1.0) > 1e-3 and abs(nu / d["stop_translation"] - 1.0) > 1e-3
        n = -(-cam["width"] // d["stride"]) * -(-cam["height"] // d["stride"])
        assert st2["points"].shape == (n, 3) and st2["valid_pixels"] == int(np.isfinite(st2["points"]).all(1).sum())
        assert st2["inliers"] <= st2["valid"] <= st2["valid_pixels"] <= n


def test_twin_returns_to_the_render_pose_and_sets_the_bars():
    worst = [0.0, 0.0]
    for key, i in SC.TRUTH_RUNS:
        g, cam, depth, start, runs, _ = SC.checked_frame(key)
        desc, pose, st = runs[i]
        s_ang, s_tr = ST.pose_err(start, cam["pose"], VS)
        ang, tr = ST.pose_err(pose, cam["pose"], VS)
        b_ang, b_tr, (o_ang, o_tr) = SC.order_bar(key, i)
        print(f"{key} {desc}: {st['valid_pixels']} usable, {st['iterations']} steps, ratio {st['min_pivot_ratio']:.2e}, against the render pose {ang:.3e} rad {tr:.3e} "
              f"voxel, rms {st['rms_initial']:.2e} -> {st['rms_final']:.2e}, sequential against numpy sums {o_ang:.2e} rad {o_tr:.2e} voxel")
        assert abs(np.degrees(s_ang) - SC.START_ROT_DEG) < 1e-6 and 0.3 < s_tr < 3.0
        assert st["status"] == 0 and 2 <= st["iterations"] <= 10 and st["inliers"] == st["valid"] == st["valid_pixels"] >= 100
        assert st["min_pivot_ratio"] >= 1e-4
        assert ang <= 0.5 * SC.TRUTH_BAR_RAD and tr <= 0.5 * SC.TRUTH_BAR_VOX                      # the device's bar is twice the twin's figure, rounded up
        assert b_ang <= 1e-9 and b_tr <= 1e-6                                                       # the order of the sums moves the pose by rounding only
        worst = [max(worst[0], ang), max(worst[1], tr)]
    print(f"worst against the render pose: {worst[0]:.3e} rad, {worst[1]:.3e} voxel")
    assert worst[0] > 0.2 * SC.TRUTH_BAR_RAD and worst[1] > 0.2 * SC.TRUTH_BAR_VOX                  # the recorded bars are not stale


def test_twin_equals_register_twin_on_the_filtered_points():
    for key in (("plain", "plain32", True, False), ("shifted", "dist32", True, False), ("negative", "plain32", False, False)):
        g, cam, depth, start, runs, _ = SC.checked_frame(key)
        grid = Q.twin_grid(g, key[2])
        desc, pose, st = runs[0]
        pts = SC.host_points(depth, cam)
        assert pts.shape[0] == st["valid_pixels"]
        r_pose, r_st = RT.register(grid, pts, RT.rt_to_pose(*ST.pose_to_cw(start)))
        b_ang, b_tr, _ = SC.order_bar(key, 0)
        ang, tr = ST.pose_err(pose, track_twin.cw_to_pose(*RT.pose_to_rt(r_pose)), VS)
        print(f"{key}: against register_twin on {pts.shape[0]} filtered points {ang:.2e} rad {tr:.2e} voxel (bar {b_ang:.1e} / {b_tr:.1e})")
        assert r_st["status"] == st["status"] == 0 and r_st["iterations"] == st["iterations"]
        assert r_st["valid"] == st["valid"] and r_st["inliers"] == st["inliers"]
        assert ang <= b_ang and (tr <= b_tr or (b_tr <= 1e-12 and SC.translation_quantum(pose) >= 1e-12))


def test_sums_orders_ragged_edges_and_ignored_pixels():
    key = ("plain", "plain32", True, False)
    g, cam, depth, start, runs, _ = SC.checked_frame(key)
    grid = Q.twin_grid(g, True)
    st = runs[0][2]
    pts, c = st["points"], st["pivot"]
    R, t = ST.pose_to_cw(start)
    for hub in (0.0, SC.HUBER):
        a = ST.sums(grid, pts, R, t - c, c, 0.05, hub)
        b = ST.sums(grid, pts, R, t - c, c, 0.05, hub, order="sequential")
        assert a["valid"] == b["valid"] and a["inliers"] == b["inliers"] and a["usable"] == st["valid_pixels"]
        assert np.all(np.abs(a["sums"] - b["sums"]) <= pts.shape[0] * 2.0 ** -52 * a["abs_sums"])
    plain, hub = ST.sums(grid, pts, R, t - c, c, 0.05), ST.sums(grid, pts, R, t - c, c, 0.05, SC.HUBER)
    assert (hub["weight"] < 1.0).sum() > 10 and hub["weight"].min() > 0.0                           # the weight acts at the start
    assert np.array_equal(plain["sums"][27:], hub["sums"][27:]) and not np.array_equal(plain["sums"][:27], hub["sums"][:27])      # r^2 and the count stay unweighted
    # stride 3 does not divide 32: 11 x 8 samples, the last column is pixel 30
    idx = ST.sample_index(32, 24, 3)
    assert idx.size == 88 and idx[10] == 30 and idx[11] == 3 * 32 and idx[-1] == 21 * 32 + 30
    assert ST.sample_index(65, 1, 2).size == 33 and ST.sample_index(1, 1, 16).tolist() == [0]
    # NaN / Inf / negative depths in place of zeros change nothing
    odd = depth.copy().reshape(-1)
    zero = np.nonzero(odd == 0)[0]
    odd[zero[0::3]] = np.nan; odd[zero[1::3]] = np.inf; odd[zero[2::3]] = -1.0
    p2, ok2, _ = ST.samples(odd.reshape(depth.shape), cam["intr"], cam["dist"])
    assert np.array_equal(np.isnan(p2), np.isnan(pts)) and np.array_equal(p2[ok2], pts[ok2])
    # the depth range
    lo = float(np.median(depth[depth > 0]))
    p3, ok3, _ = ST.samples(depth, cam["intr"], cam["dist"], 1, lo, 0.0)
    assert 0 < ok3.sum() < ok2.sum() and np.array_equal(ok3, depth.reshape(-1) >= np.float32(lo))
    # statuses of the loop
    empty = ST.track(grid, np.zeros_like(depth), cam["intr"], cam["dist"], start)
    assert empty[1]["status"] == 2 and empty[1]["valid_pixels"] == 0 and np.array_equal(empty[0], start)
    p1, s1 = ST.track(grid, depth, cam["intr"], cam["dist"], start, dict(iterations=1))
    assert s1["status"] == 1 and s1["iterations"] == 1 and not np.array_equal(p1, start)
    p0, s0 = ST.track(grid, depth, cam["intr"], cam["dist"], start, dict(iterations=0))
    assert s0["status"] == 1 and np.array_equal(p0, start) and s0["rms_initial"] == s0["rms_final"] == st["rms_initial"]


def test_twin_rotation_is_the_drivers_formula():
    """track_sdf_twin.rotation restates frame_math.hpp's rotation; it must be a rotation and agree with synthetic.aa_to_rotmat to rounding"""
    from intrinsic3d_amd import synthetic
    rng = np.random.default_rng(1)
    for aa in list(rng.normal(size=(20, 3))) + [np.zeros(3), np.array([1e-9, 0.0, 0.0]), np.array([0.0, 3.0, 0.5])]:
        R = ST.rotation(aa)
        assert np.abs(R - synthetic.aa_to_rotmat(aa)).max() <= 8 * 2.0 ** -52 and np.abs(R @ R.T - np.eye(3)).max() <= 8 * 2.0 ** -52
    p = np.array([0.3, -0.2, 0.5, 1.0, -2.0, 400.0])
    Rc, tc = ST.pose_to_cw(p)
    assert np.array_equal(Rc.T, ST.rotation(p[:3])) and np.abs(Rc.T @ tc + p[3:]).max() <= 1e-12


def test_huber_input_condition():
    """the corrupted frame: 20 % of the usable pixels 1.5 voxels deeper, inside the default gate; the weight must bring the twin closer to the render pose"""
    key = ("plain", "plain32", True, True)
    g, cam, depth, start, runs, _ = SC.checked_frame(key)
    clean = SC.rendered("plain", "plain32", True)
    moved = np.nonzero((depth != clean) & (depth > 0))
    deeper = (depth[moved].astype(np.float64) - clean[moved]) / VS
    share = moved[0].size / float((clean > 0).sum())
    assert abs(share - SC.CORRUPT_SHARE) < 0.01 and np.all(np.abs(deeper - SC.CORRUPT_VOX) < 1e-3)
    (d_off, p_off, s_off), (d_on, p_on, s_on) = runs
    assert "huber_delta" not in d_off and d_on["huber_delta"] == SC.HUBER == 0.5 * VS
    assert s_off["valid"] == s_off["inliers"] and s_on["valid"] == s_on["inliers"]                  # the outliers stay inside the default gate
    e_off, e_on = ST.pose_err(p_off, cam["pose"], VS), ST.pose_err(p_on, cam["pose"], VS)
    print(f"corrupted frame: huber off {e_off[0]:.3e} rad {e_off[1]:.3e} voxel ({s_off['iterations']} steps), huber_delta = vs / 2 {e_on[0]:.3e} rad {e_on[1]:.3e} voxel "
          f"({s_on['iterations']} steps)")
    assert s_off["status"] == s_on["status"] == 0
    assert e_on[0] < e_off[0] and e_on[1] < e_off[1]


def test_track_sdf_struct_layouts_match_header():
    """ctypes mirrors must have the C struct sizes and offsets (checked against a tiny C program compiled with gcc)."""
    binding, L = _lib()
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "intrinsic3d_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(i3d_track_sdf_desc), '
           'sizeof(i3d_track_sdf_stats), offsetof(i3d_track_sdf_desc, distortion5), offsetof(i3d_track_sdf_desc, stride), offsetof(i3d_track_sdf_desc, huber_delta), '
           'offsetof(i3d_track_sdf_desc, max_depth), offsetof(i3d_track_sdf_desc, stop_translation), offsetof(i3d_track_sdf_stats, valid), '
           'offsetof(i3d_track_sdf_stats, min_pivot_ratio));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        sizes = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    D, S = binding.TrackSdfDesc, binding.TrackSdfStats
    assert sizes == [C.sizeof(D), C.sizeof(S), D.distortion5.offset, D.stride.offset, D.huber_delta.offset, D.max_depth.offset, D.stop_translation.offset,
                     S.valid.offset, S.min_pivot_ratio.offset]


def test_symbols_defaults_and_argument_errors_without_a_device():
    binding, L = _lib()
    for s in ("i3d_track_sdf_desc_default", "i3d_track_frame_sdf", "i3d_fusion_track_sdf", "i3d_debug_track_sdf_sums"):
        assert hasattr(L, s) and s in binding.EXPORTS, s
    d = binding.track_sdf_desc_default()
    assert (d.use_refined_sdf, d.use_context_camera, d.iterations, d.stride, d.max_distance, d.huber_delta, d.min_depth, d.max_depth, d.stop_rotation,
            d.stop_translation) == (1, 0, 30, 1, 0.05, 0.0, 0.0, 0.0, 1e-6, 1e-6)
    tw = ST.default_desc()
    assert all(tw[k] == getattr(d, k) for k in tw)
    d2 = binding.track_sdf_desc_default(refined=False, intr=[1, 2, 3, 4], dist=[5, 6, 7, 8, 9], stride=4, huber_delta=0.01)
    assert (d2.use_refined_sdf, list(d2.intrinsics4), list(d2.distortion5), d2.stride, d2.huber_delta) == (0, [1, 2, 3, 4], [5, 6, 7, 8, 9], 4, 0.01)
    with pytest.raises(ValueError):
        binding.track_sdf_desc_default(levels=2)
    L.i3d_track_sdf_desc_default(None)                            # a null descriptor is ignored
    dep = np.zeros((2, 2), np.float32); pose = np.zeros(6); sums = np.zeros(29); p = binding._p
    st = binding.TrackSdfStats()
    assert L.i3d_track_frame_sdf(None, d, 2, 2, p(dep), p(pose), C.byref(st)) == 1                  # I3D_ERR_INVALID_ARGUMENT: a null handle
    assert L.i3d_fusion_track_sdf(None, d, 2, 2, p(dep), p(pose), C.byref(st)) == 1
    assert L.i3d_debug_track_sdf_sums(None, d, 2, 2, p(dep), p(pose), p(pose[:3].copy()), p(sums), None, None) == 1
