"""i3d_track_frame on the device: the association sums against their numpy statement (track_twin.py), convergence on a scene that pins all six DoF,
reproducibility, what it must leave alone, the errors, and the CLI's opt-in output of tracked poses."""
import os
import subprocess
import sys

import numpy as np
import pytest

import track_cases as TC
import track_twin
from intrinsic3d_amd import binding, synthetic
from track_cases import BUMPY, CASES, DIST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", list(CASES))
def test_sums_match_twin(case):
    kw = CASES[case]
    sc = TC.scene(shift=kw.get("shift"))
    dist = kw.get("dist")
    ctx = TC.context(sc, dist)
    try:
        vs = float(sc["voxel_size"])
        depth = TC.view(ctx, sc, sc["truth"], 0, dist)[0]
        assert (depth > 0).sum() > 0.2 * depth.size
        rng = np.random.default_rng(3)
        pose_ref = track_twin.perturb(sc["truth"], rng, 0.7, 1.5 * vs)
        pose_cur = track_twin.perturb(sc["truth"], rng, 0.5, 1.0 * vs)
        pyr = track_twin.depth_pyramid(depth, 2)
        for level in (0, 1):
            sums, n = ctx.debug_track_sums(depth, level, pose_ref, pose_cur, levels=2)
            cam = track_twin.level_camera(sc["intr"], np.zeros(5) if dist is None else dist, sc["width"], sc["height"], level)
            md, mn = TC.view(ctx, sc, pose_ref, level, dist)
            vtx, nrm = track_twin.frame_points(pyr[level], cam)
            Rc, tc = track_twin.pose_to_cw(pose_cur)
            tw = track_twin.associate(vtx, nrm, md, mn, cam, track_twin.ref_from_pose(pose_ref), Rc, tc, 0.05, 0.8)
            assert tw["inliers"] > 300
            flips = abs(n - tw["inliers"])
            assert flips <= 0.001 * cam["w"] * cam["h"], (n, tw["inliers"])
            assert sums[28] == n
            if flips == 0:
                assert np.all(np.abs(sums - tw["sums"]) <= 1e-9 * tw["abs_sums"]), np.max(np.abs(sums - tw["sums"]) / tw["abs_sums"])
            else:                                     # a pixel at a gate went the other way: its terms are the difference
                per = tw["abs_sums"] / tw["inliers"]
                assert np.all(np.abs(sums - tw["sums"]) <= 1e-9 * tw["abs_sums"] + 50.0 * flips * per)
    finally:
        ctx.close()


def test_converges_to_the_true_pose():
    sc = TC.scene()
    ctx = TC.context(sc)
    try:
        vs = float(sc["voxel_size"])
        depth = TC.view(ctx, sc, sc["truth"])[0]
        rng = np.random.default_rng(17)
        for _ in range(3):
            start = track_twin.perturb(sc["truth"], rng, 2.0, 3.0 * vs)
            pose, st = ctx.track_frame(depth, start)
            r, c = track_twin.rot_err_deg(pose, sc["truth"]), track_twin.centre_err(pose, sc["truth"]) / vs
            assert st["status"] == 0 and r < 0.02 and c < 0.05, (r, c, st)
            assert st["min_pivot_ratio"] > 1e-4, st                 # the bumps pin all six DoF
            assert st["rms_final"] < st["rms_initial"] and st["inliers"] > 0.5 * (depth > 0).sum()
        pose, st = ctx.track_frame(depth, sc["truth"])
        assert st["status"] == 0 and track_twin.centre_err(pose, sc["truth"]) < 1e-3 * vs and track_twin.rot_err_deg(pose, sc["truth"]) < 1e-3, st
    finally:
        ctx.close()


def test_deterministic():
    sc = TC.scene(seed=8)
    ctx = TC.context(sc, DIST)
    try:
        depth = TC.view(ctx, sc, sc["truth"], 0, DIST)[0]
        start = track_twin.perturb(sc["truth"], np.random.default_rng(5), 1.5, 2.0 * float(sc["voxel_size"]))
        a = ctx.track_frame(depth, start, levels=3)
        b = ctx.track_frame(depth, start, levels=3)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    finally:
        ctx.close()


def test_tracking_changes_nothing():
    sc = TC.scene(seed=9)
    vs = float(sc["voxel_size"])
    rng = np.random.default_rng(11)
    sdf_r = sc["sdf"].astype(np.float64) + rng.normal(0.0, 0.05 * vs, sc["keys"].shape[0])
    cfg = binding.default_config(iterations=1, thres_shell=2.0 * vs)
    results = []
    for track in (False, True):
        ctx = TC.context(sc, sdf_refined=sdf_r)
        try:
            ctx.estimate_sh(0.05, 10.0, 2.0 * vs)
            depth = TC.view(ctx, sc, sc["truth"])[0]
            stats = []
            for _ in range(2):
                if track:
                    ctx.track_frame(depth, track_twin.perturb(sc["truth"], np.random.default_rng(1), 1.0, vs))
                stats += ctx.optimize(cfg)
            results.append((ctx.export_grid(), ctx.get_camera(), stats))
        finally:
            ctx.close()
    (g0, c0, s0), (g1, c1, s1) = results
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
    for a, b in zip(c0, c1):
        assert np.array_equal(a, b)
    for a, b in zip(s0, s1):
        for name, _ in binding.IterationStats._fields_:
            if not name.startswith("time_"):
                x, y = getattr(a, name), getattr(b, name)
                assert (list(x) == list(y)) if hasattr(x, "__len__") else x == y, name


def test_track_errors():
    sc = TC.scene()
    depth = np.ones((sc["height"], sc["width"]), np.float32)
    with binding.Context(0) as ctx:
        assert TC.rc(lambda: ctx.track_frame(depth, sc["truth"])) == 4                      # no grid
        ctx.set_grid(sc["voxel_size"], sc["keys"], sc["sdf"], sc["sdf"], sc["albedo_true"], sc["weight"], sc["color"])
        assert TC.rc(lambda: ctx.track_frame(depth, sc["truth"])) == 4                      # use_context_camera without a camera
        depth = ctx.render_view(frame=-1, planes=("depth",), camera=dict(width=sc["width"], height=sc["height"], intr=sc["intr"], pose=sc["truth"]))["depth"]
        pose, st = ctx.track_frame(depth, sc["truth"], intr=sc["intr"])                   # a fused grid and a camera of its own: no keyframes, no SH
        assert st["status"] == 0
        ctx.set_frames(sc["frames"], sc["levels"])
        ctx.set_camera(sc["intr"], np.zeros(5), sc["poses"])
        for bad in (dict(levels=0), dict(levels=5), dict(iterations=[101]), dict(iterations=[-1]), dict(max_distance=0.0)):
            assert TC.rc(lambda: ctx.track_frame(depth, sc["truth"], **bad)) == 1, bad
        assert TC.rc(lambda: ctx.track_frame(np.zeros((0, 4), np.float32), sc["truth"])) == 1
        assert TC.rc(lambda: ctx.track_frame(depth[:12, :12], sc["truth"], levels=3)) == 1  # too small for three levels
        d = binding.track_desc_default()
        pose = np.array(sc["truth"], np.float64); st = binding.TrackStats()
        assert ctx.L.i3d_track_frame(ctx.h, d, sc["width"], sc["height"], None, binding._p(pose), st) == 1
        pose, st = ctx.track_frame(np.zeros_like(depth), sc["truth"])
        assert st["status"] == 2 and np.array_equal(pose, np.asarray(sc["truth"], np.float64))


def test_cli_tracked_poses(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_dataset
    app = os.path.join(ROOT, "apps", "app_intrinsic3d")
    assert os.path.exists(app), "apps/app_intrinsic3d has not been built (run __graft_entry__.build())"
    sc = synthetic.make_scene(radius_vox=14, K=6, width=128, height=96, levels=1, seed=9, lum_noise=0.003, **BUMPY)
    cam = track_twin.level_camera(sc["intr"], np.zeros(5), sc["width"], sc["height"], 0)
    for f, fr in enumerate(sc["frames"]):             # render_frame's depth is the base sphere: give the frames the bumpy surface the model holds
        fr["depth"][0] = track_twin.raycast_scene(sc["scene"], cam, track_twin.ref_from_pose(sc["poses"][f]))[0]
    plain = tmp_path / "plain"; keyed = tmp_path / "keyed"
    s0, i0 = make_dataset.write_dataset(str(plain), sc, grid_levels=2, rgbd_levels=1, iterations=2, extra_frames=3)
    s1, i1 = make_dataset.write_dataset(str(keyed), sc, grid_levels=2, rgbd_levels=1, iterations=2, extra_frames=3,
                                        output_tracked_poses_prefix="./intrinsic3d/tracked")
    for s, i in ((s0, i0), (s1, i1)):
        r = subprocess.run([app, "-s", s, "-i", i], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
    assert not list((plain / "intrinsic3d").glob("tracked*"))
    assert sorted(p.name for p in (keyed / "intrinsic3d").glob("tracked*")) == ["tracked_g0_p0.txt", "tracked_g1_p0.txt"]
    for name in ("poses_g1_p0.txt", "poses_g0_p0.txt"):                                    # the sensor's poses are what they were without the key
        assert np.array_equal(np.loadtxt(plain / "intrinsic3d" / name), np.loadtxt(keyed / "intrinsic3d" / name)), name
    tracked = np.loadtxt(keyed / "intrinsic3d" / "tracked_g0_p0.txt")
    poses = np.loadtxt(keyed / "intrinsic3d" / "poses_g0_p0.txt")
    assert tracked.shape == poses.shape == (9, 8)
    assert np.array_equal(tracked[:6], poses[:6])                                           # keyframes: their refined poses
    assert np.all(np.isfinite(tracked))
    # the extra frames repeat the last keyframe's image and input pose: the guess is that keyframe's refined pose, and registration stays within a few voxels
    vs = float(sc["voxel_size"])
    for i in range(6, 9):
        assert np.linalg.norm(tracked[i, 1:4] - poses[5, 1:4]) < 3.0 * vs
        assert abs(abs(np.dot(tracked[i, 4:], poses[5, 4:])) - 1.0) < 1e-3
