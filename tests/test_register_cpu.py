"""-m "not gpu": the numpy statement of i3d_register_points (register_twin.py) on the checked point sets of register_cases.py - the input conditions the device
comparison relies on, the bars it is held to - and what the entry points do without a device: struct layouts, symbols, defaults, argument errors."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import query_cases as Q
import query_twin
import register_cases as RC
import register_twin as RT
import render_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [(name, refined) for name in RC.GRID_NAMES for refined in (True, False)]


def _lib():
    from intrinsic3d_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return binding, binding.load()


@pytest.mark.parametrize("name,refined", CASES)
def test_checked_sets_meet_the_input_conditions(name, refined):
    g, pts, runs = RC.checked_set(name, refined)
    grid = Q.twin_grid(g, refined)
    assert pts.shape == (RC.N_FULL, 3)
    truth = RC.true_pose(g)
    md = RT.default_desc()["max_distance"]
    on = RT.sums(grid, pts, *RT.pose_to_rt(truth)[:1], RT.pose_to_rt(truth)[1] - RT.pivot(grid, pts, truth), RT.pivot(grid, pts, truth), md)
    assert on["inliers"] == RC.N_FULL and np.abs(on["r"]).max() <= 1e-5 * RC.VS        # the points lie on the model's zero set at the true pose
    for k, (start, pose, st) in enumerate(runs):
        again, st2 = RT.register(grid, pts, start, trace=True)                           # the set as the device test will see it
        assert np.array_equal(again, pose)
        face, gate = RC.run_margins(grid, pts, st2, md)
        assert face.min() >= RC.FACE_MARGIN and gate.min() >= RC.GATE_MARGIN
        assert st2["status"] == 0 and 2 <= st2["iterations"] <= 10
        assert st2["min_pivot_ratio"] >= 1e-3, st2["min_pivot_ratio"]                    # all six degrees of freedom are pinned
        assert st2["valid"] == st2["inliers"] == RC.N_FULL and st2["rms_final"] < 1e-3 * st2["rms_initial"]
        d = RT.default_desc()
        for nw, nu in st2["steps"]:                                                       # no step sits on the stop rule
            assert abs(nw / d["stop_rotation"] - 1.0) > RC.STOP_MARGIN and abs(nu / d["stop_translation"] - 1.0) > RC.STOP_MARGIN
        s_ang, s_tr = RT.pose_diff(start, truth, RC.VS)
        assert abs(np.degrees(s_ang) - RC.START_ROT_DEG) < 1e-6 and 0.5 < s_tr < 30.0    # 1 degree about the sphere's centre, 1.5 voxels
        ang, tr = RT.pose_diff(pose, truth, RC.VS)
        b_ang, b_tr, (o_ang, o_tr) = RC.twin_order_bar(name, refined, k)
        print(f"{name} refined={refined} start {k}: {st2['iterations']} steps, ratio {st2['min_pivot_ratio']:.2e}, against the truth {ang:.2e} rad {tr:.2e} voxel, "
              f"sequential against numpy sums {o_ang:.2e} rad {o_tr:.2e} voxel")
        assert ang <= 0.5 * RC.TRUTH_BAR_RAD and tr <= 0.5 * RC.TRUTH_BAR_VOX          # the device's bar is twice the twin's figure, rounded up
        assert b_ang <= 1e-9 and b_tr <= 1e-8                                             # the order of the sums moves the pose by rounding only


def test_sums_terms_and_special_points():
    g, pts, runs = RC.checked_set("plain", True)
    grid = Q.twin_grid(g, True)
    start = runs[0][0]
    c = RT.pivot(grid, pts, start)
    R, t = RT.pose_to_rt(start)
    md = RT.default_desc()["max_distance"]
    a = RT.sums(grid, pts, R, t - c, c, md)
    b = RT.sums(grid, pts, R, t - c, c, md, order="sequential")
    assert a["valid"] == b["valid"] == a["inliers"] == b["inliers"] and 1500 < a["valid"] <= RC.N_FULL      # at the start some points lie outside the band
    assert np.all(np.abs(a["sums"] - b["sums"]) <= RC.N_FULL * 2.0 ** -52 * a["abs_sums"])
    # special points are never valid and do not move the pivot
    both = np.concatenate([pts, RC.SPECIAL])
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.array_equal(RT.pivot(grid, both, start), c)
        s = RT.sums(grid, both, R, t - c, c, md)
    assert not s["valid_mask"][RC.N_FULL:].any() and np.array_equal(s["sums"], a["sums"])
    # empty space: nothing valid; a tight gate: valid but fewer inliers
    e = RT.sums(grid, RC.empty_points(g, 500, 3), R, t - c, c, md)
    assert e["valid"] == 0 and e["inliers"] == 0
    tight = RT.sums(grid, pts, R, t - c, c, 0.5 * RC.VS)
    assert tight["valid"] == a["valid"] and 64 < tight["inliers"] < a["valid"]
    # statuses of the loop
    assert RT.register(grid, pts[:63], start)[1]["status"] == 2 and RT.register(grid, np.zeros((0, 3)), start)[1]["status"] == 2
    p1, s1 = RT.register(grid, pts, start, dict(iterations=1))
    assert s1["status"] == 1 and s1["iterations"] == 1 and not np.array_equal(p1, start)
    p0, s0 = RT.register(grid, pts, start, dict(iterations=0))
    assert s0["status"] == 1 and s0["iterations"] == 0 and np.array_equal(p0, start) and s0["rms_initial"] == s0["rms_final"] == runs[0][2]["rms_initial"]


def test_depth_frame_case():
    g = RC.grid("plain")
    grid = Q.twin_grid(g, True)
    cam = Q.view_camera(g)
    rt = render_twin.render(grid, render_twin.camera_from_pose(cam["pose"], cam["intr"], cam["dist"], cam["width"], cam["height"]))
    pts, truth, start = RC.view_case(g, rt["depth"].astype(np.float32))
    assert pts.shape[0] > 200
    pose, st = RT.register(grid, pts, start)
    ang, tr = RT.pose_diff(pose, truth, RC.VS)
    s_ang, s_tr = RT.pose_diff(start, truth, RC.VS)
    print(f"view: {pts.shape[0]} points, start {s_ang:.2e} rad {s_tr:.2e} voxel, {st['iterations']} steps, status {st['status']}, ratio {st['min_pivot_ratio']:.2e}, "
          f"returns within {ang:.2e} rad {tr:.2e} voxel, rms {st['rms_initial']:.2e} -> {st['rms_final']:.2e}")
    assert st["status"] == 0 and st["inliers"] == pts.shape[0]
    assert ang <= 0.5 * RC.VIEW_BAR_RAD and tr <= 0.5 * RC.VIEW_BAR_VOX


def test_register_struct_layouts_match_header():
    """ctypes mirrors must have the C struct sizes (checked against a tiny C program compiled with gcc)."""
    binding, L = _lib()
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "intrinsic3d_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(i3d_register_desc), '
           'sizeof(i3d_register_stats), offsetof(i3d_register_desc, max_distance), offsetof(i3d_register_desc, stop_translation), '
           'offsetof(i3d_register_stats, valid), offsetof(i3d_register_stats, min_pivot_ratio));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        sizes = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    D, S = binding.RegisterDesc, binding.RegisterStats
    assert sizes == [C.sizeof(D), C.sizeof(S), D.max_distance.offset, D.stop_translation.offset, S.valid.offset, S.min_pivot_ratio.offset]


def test_symbols_defaults_and_argument_errors_without_a_device():
    binding, L = _lib()
    for s in ("i3d_register_desc_default", "i3d_register_points", "i3d_fusion_register_points", "i3d_debug_register_sums", "i3d_debug_register_row_cap"):
        assert hasattr(L, s) and s in binding.EXPORTS, s
    d = binding.register_desc_default()
    assert (d.use_refined_sdf, d.iterations, d.max_distance, d.stop_rotation, d.stop_translation) == (1, 30, 0.05, 1e-6, 1e-6)
    tw = RT.default_desc()
    assert (tw["iterations"], tw["max_distance"], tw["stop_rotation"], tw["stop_translation"]) == (d.iterations, d.max_distance, d.stop_rotation, d.stop_translation)
    d2 = binding.register_desc_default(refined=False, iterations=7, max_distance=0.01)
    assert (d2.use_refined_sdf, d2.iterations, d2.max_distance) == (0, 7, 0.01)
    with pytest.raises(ValueError):
        binding.register_desc_default(levels=2)
    L.i3d_register_desc_default(None)                             # a null descriptor is ignored
    pts = np.zeros((4, 3)); pose = np.zeros(6); sums = np.zeros(29); p = binding._p
    st = binding.RegisterStats()
    assert L.i3d_register_points(None, d, 4, p(pts), p(pose), C.byref(st)) == 1          # I3D_ERR_INVALID_ARGUMENT: a null handle
    assert L.i3d_fusion_register_points(None, d, 4, p(pts), p(pose), C.byref(st)) == 1
    assert L.i3d_debug_register_sums(None, d, 4, p(pts), p(pose), p(pose[:3].copy()), p(sums), None) == 1
    assert L.i3d_debug_register_row_cap(None, 8) == 1
