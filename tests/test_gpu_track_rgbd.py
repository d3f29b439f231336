"""i3d_track_frame_rgbd on the device: the combined sums against their numpy statement (track_rgbd_twin.py), the reduction to i3d_track_frame, a smooth sphere
that only colour can register, the bumpy scene that depth already registered, reproducibility, what it must leave alone, the errors, and the CLI's opt-in key.
Scenes are those of test_gpu_track.py with the true albedo in the grid and the scene's SH at every voxel; a frame is the model's own depth and intensity cast
at the true pose.  The smooth scene, its starts, the descriptor and the reason for its stop rule are in track_cases.py; test_track_rgbd_cpu.py holds the twin to a
fifth of the bars used here."""
import os
import subprocess
import sys

import numpy as np
import pytest

import track_cases as TC
import track_rgbd_twin as rgbd_twin
import track_twin
from intrinsic3d_amd import binding, synthetic
from track_cases import BAR_DEG, BAR_VOX, BUMPY, CASES, DESC, DIST, WEIGHTS, smooth_scene, smooth_starts, voxel_sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _view(ctx, sc, pose, level=0, dist=None):
    """the model ray-cast through the renderer: (depth, world normal, intensity) of the level's camera"""
    cam = track_twin.level_camera(sc["intr"], np.zeros(5) if dist is None else dist, sc["width"], sc["height"], level)
    out = ctx.render_view(frame=-1, planes=("depth", "normal", "intensity"), camera=dict(width=cam["w"], height=cam["h"], intr=cam["intr"], dist=cam["dist"], pose=pose))
    return out["depth"], out["normal"], out["intensity"]


def _errors(pose, sc):
    return track_twin.rot_err_deg(pose, sc["truth"]), track_twin.centre_err(pose, sc["truth"]) / float(sc["voxel_size"])


@pytest.mark.parametrize("case", list(CASES))
def test_rgbd_sums_match_twin(case):
    kw = CASES[case]
    sc = TC.scene(shift=kw.get("shift"))
    dist = kw.get("dist")
    ctx = TC.rgbd_context(sc, dist)
    try:
        vs = float(sc["voxel_size"])
        depth, _, lum = _view(ctx, sc, sc["truth"], 0, dist)
        assert (depth > 0).sum() > 0.2 * depth.size
        rng = np.random.default_rng(3)
        pose_ref = track_twin.perturb(sc["truth"], rng, 0.7, 1.5 * vs)
        pose_cur = track_twin.perturb(sc["truth"], rng, 0.5, 1.0 * vs)
        pyr = track_twin.depth_pyramid(depth, 2); lpyr = rgbd_twin.lum_pyramid(lum, 2)
        for level in (0, 1):
            cam = track_twin.level_camera(sc["intr"], np.zeros(5) if dist is None else dist, sc["width"], sc["height"], level)
            md, mn, mi = _view(ctx, sc, pose_ref, level, dist)
            vtx, nrm = track_twin.frame_points(pyr[level], cam)
            Rc, tc = track_twin.pose_to_cw(pose_cur)
            for wg, wp in ((0.0, 1.0), (1.0, 0.1)):                       # photometric only, mixed
                sums, n, m = ctx.debug_track_rgbd_sums(depth, lum, level, pose_ref, pose_cur, levels=2, geometric_weight=wg, photo_weight=wp)
                tw = rgbd_twin.associate_rgbd(vtx, nrm, md, mn, mi, lpyr[level], cam, track_twin.ref_from_pose(pose_ref), Rc, tc, 0.05, 0.8, wg, wp)
                print(case, level, wg, wp, "inliers", n, tw["inliers"], "samples", m, tw["samples"], "max rel", np.max(np.abs(sums - tw["sums"]) / np.maximum(tw["abs_sums"], 1e-300)))
                assert tw["inliers"] > 300 and tw["samples"] > 300
                flips = abs(n - tw["inliers"]) + abs(m - tw["samples"])
                assert flips <= 0.001 * cam["w"] * cam["h"], (n, tw["inliers"], m, tw["samples"])
                assert sums[28] == n and sums[30] == m
                if flips == 0:
                    assert np.all(np.abs(sums - tw["sums"]) <= 1e-9 * tw["abs_sums"]), np.max(np.abs(sums - tw["sums"]) / np.maximum(tw["abs_sums"], 1e-300))
                else:                                     # a pixel at a gate went the other way: its terms are the difference
                    per = tw["abs_sums"] / min(tw["inliers"], tw["samples"])
                    assert np.all(np.abs(sums - tw["sums"]) <= 1e-9 * tw["abs_sums"] + 50.0 * flips * per)
    finally:
        ctx.close()


def test_reduces_to_the_depth_only_tracker():
    sc = TC.scene()
    ctx = TC.rgbd_context(sc, DIST)
    try:
        vs = float(sc["voxel_size"])
        depth, _, lum = _view(ctx, sc, sc["truth"], 0, DIST)
        rng = np.random.default_rng(3)
        pose_ref = track_twin.perturb(sc["truth"], rng, 0.7, 1.5 * vs)
        pose_cur = track_twin.perturb(sc["truth"], rng, 0.5, 1.0 * vs)
        for level in (0, 1):
            old, n_old = ctx.debug_track_sums(depth, level, pose_ref, pose_cur, levels=2)
            new, n_new, m = ctx.debug_track_rgbd_sums(depth, lum, level, pose_ref, pose_cur, levels=2, geometric_weight=1.0, photo_weight=0.0)
            assert n_old == n_new and m == 0 and old.tobytes() == new[:29].tobytes() and new[29] == 0.0 and new[30] == 0.0
        for seed in (17, 18):
            start = track_twin.perturb(sc["truth"], np.random.default_rng(seed), 2.0, 3.0 * vs)
            pose_o, st_o = ctx.track_frame(depth, start, levels=2)
            pose_n, st_n = ctx.track_frame_rgbd(depth, lum, start, levels=2, geometric_weight=1.0, photo_weight=0.0)
            assert pose_o.tobytes() == pose_n.tobytes()
            assert {k: st_n[k] for k in st_o} == st_o and st_n["photo_samples"] == 0
    finally:
        ctx.close()


def test_colour_pins_what_depth_cannot():
    sc = smooth_scene()
    ctx = TC.rgbd_context(sc)
    try:
        depth, _, lum = _view(ctx, sc, sc["truth"])
        for start in smooth_starts(sc):
            pose_c, st_c = ctx.track_frame_rgbd(depth, lum, start, **DESC, **WEIGHTS)
            pose_d, st_d = ctx.track_frame(depth, start, **DESC)
            (rc, cc), (rd, cd) = _errors(pose_c, sc), _errors(pose_d, sc)
            print(f"rgbd {rc:.5f} deg {cc:.5f} voxel {st_c}\ndepth only {rd:.4f} deg {cd:.4f} voxel {st_d}")
            assert st_c["status"] == 0 and rc < BAR_DEG and cc < BAR_VOX, (rc, cc, st_c)
            assert rd >= 10.0 * rc, (rd, rc)
            assert st_c["min_pivot_ratio"] > st_d["min_pivot_ratio"], (st_c, st_d)
            assert st_c["photo_samples"] > 0.9 * st_c["inliers"] and st_c["photo_rms_final"] < st_c["photo_rms_initial"]
    finally:
        ctx.close()


def test_still_converges_where_depth_already_did():
    sc = TC.scene()
    ctx = TC.rgbd_context(sc)
    try:
        vs = float(sc["voxel_size"])
        depth, _, lum = _view(ctx, sc, sc["truth"])
        rng = np.random.default_rng(17)
        for _ in range(3):                                # the starts of test_gpu_track.py::test_converges_to_the_true_pose
            start = track_twin.perturb(sc["truth"], rng, 2.0, 3.0 * vs)
            pose, st = ctx.track_frame_rgbd(depth, lum, start, **DESC, **WEIGHTS)
            r, c = _errors(pose, sc)
            print(f"{r:.5f} deg {c:.5f} voxel {st}")
            assert st["status"] == 0 and r < BAR_DEG and c < BAR_VOX, (r, c, st)
            assert st["rms_final"] < st["rms_initial"] and st["inliers"] > 0.5 * (depth > 0).sum()
    finally:
        ctx.close()


def test_rgbd_deterministic():
    sc = TC.scene(seed=8)
    ctx = TC.rgbd_context(sc, DIST)
    try:
        depth, _, lum = _view(ctx, sc, sc["truth"], 0, DIST)
        start = track_twin.perturb(sc["truth"], np.random.default_rng(5), 1.5, 2.0 * float(sc["voxel_size"]))
        a = ctx.track_frame_rgbd(depth, lum, start, levels=3, **WEIGHTS)
        b = ctx.track_frame_rgbd(depth, lum, start, levels=3, **WEIGHTS)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[1]["photo_samples"] > 0
    finally:
        ctx.close()


def test_rgbd_tracking_changes_nothing():
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
            depth, _, lum = _view(ctx, sc, sc["truth"])
            start = track_twin.perturb(sc["truth"], np.random.default_rng(1), 1.0, vs)
            before = ctx.track_frame(depth, start)
            if track:                                     # the depth-only tracker answers as before once the RGB-D one has used the shared buffers
                ctx.track_frame_rgbd(depth, lum, start, **WEIGHTS)
                after = ctx.track_frame(depth, start)
                assert np.array_equal(before[0], after[0]) and before[1] == after[1]
            stats = []
            for _ in range(2):
                if track:
                    ctx.track_frame_rgbd(depth, lum, start, **WEIGHTS)
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


def test_rgbd_errors():
    sc = TC.scene()
    depth = np.ones((sc["height"], sc["width"]), np.float32); lum = np.full_like(depth, 0.5)
    with binding.Context(0) as ctx:
        assert TC.rc(lambda: ctx.track_frame_rgbd(depth, lum, sc["truth"], **WEIGHTS)) == 4                 # no grid
        ctx.set_grid(sc["voxel_size"], sc["keys"], sc["sdf"], sc["sdf"], sc["albedo_true"], sc["weight"], sc["color"])
        assert TC.rc(lambda: ctx.track_frame_rgbd(depth, lum, sc["truth"], **WEIGHTS)) == 4                 # use_context_camera without a camera
        depth = ctx.render_view(frame=-1, planes=("depth",), camera=dict(width=sc["width"], height=sc["height"], intr=sc["intr"], pose=sc["truth"]))["depth"]
        assert TC.rc(lambda: ctx.track_frame_rgbd(depth, lum, sc["truth"], intr=sc["intr"], **WEIGHTS)) == 4   # a photometric weight without per-voxel SH
        assert TC.rc(lambda: ctx.debug_track_rgbd_sums(depth, lum, 0, sc["truth"], sc["truth"], intr=sc["intr"], **WEIGHTS)) == 4
        pose, st = ctx.track_frame_rgbd(depth, lum, sc["truth"], intr=sc["intr"], geometric_weight=1.0, photo_weight=0.0)      # no SH needed without it
        assert st["status"] == 0 and st["photo_samples"] == 0
        ctx.set_frames(sc["frames"], sc["levels"])
        ctx.set_camera(sc["intr"], np.zeros(5), sc["poses"])
        ctx.set_voxel_sh(voxel_sh(sc))
        lum = ctx.render_view(frame=-1, planes=("intensity",), camera=dict(width=sc["width"], height=sc["height"], intr=sc["intr"], pose=sc["truth"]))["intensity"]
        pose, st = ctx.track_frame_rgbd(depth, lum, sc["truth"], **WEIGHTS)
        assert st["status"] == 0 and st["photo_samples"] > 0
        for bad in (dict(geometric_weight=-1.0), dict(photo_weight=-0.1), dict(photo_weight=float("nan")), dict(geometric_weight=float("inf")),
                    dict(geometric_weight=0.0, photo_weight=0.0), dict(levels=0), dict(levels=5), dict(iterations=[101]), dict(max_distance=0.0)):
            assert TC.rc(lambda: ctx.track_frame_rgbd(depth, lum, sc["truth"], **bad)) == 1, bad
            assert TC.rc(lambda: ctx.debug_track_rgbd_sums(depth, lum, 0, sc["truth"], sc["truth"], **bad)) == 1, bad
        assert TC.rc(lambda: ctx.track_frame_rgbd(depth, None, sc["truth"], **WEIGHTS)) == 1                # null luminance
        d = binding.track_rgbd_desc_default()
        pose = np.array(sc["truth"], np.float64); st = binding.TrackRgbdStats()
        assert ctx.L.i3d_track_frame_rgbd(ctx.h, d, sc["width"], sc["height"], None, binding._p(lum), binding._p(pose), st) == 1      # null depth
        assert ctx.L.i3d_track_frame_rgbd(ctx.h, None, sc["width"], sc["height"], binding._p(depth), binding._p(lum), binding._p(pose), st) == 1
        assert ctx.L.i3d_track_frame_rgbd(ctx.h, d, sc["width"], sc["height"], binding._p(depth), binding._p(lum), None, st) == 1
        assert TC.rc(lambda: ctx.debug_track_rgbd_sums(depth, lum, 1, sc["truth"], sc["truth"])) == 1       # level out of range
        pose, st = ctx.track_frame_rgbd(np.zeros_like(depth), lum, sc["truth"], **WEIGHTS)
        assert st["status"] == 2 and np.array_equal(pose, np.asarray(sc["truth"], np.float64))
        pose, st = ctx.track_frame_rgbd(depth, np.full_like(lum, 5.0), sc["truth"], geometric_weight=0.0, photo_weight=1.0, max_photo_residual=0.01)   # every sample gated
        assert st["status"] == 2 and st["inliers"] > 64 and st["photo_samples"] < 64 and np.array_equal(pose, np.asarray(sc["truth"], np.float64))


def test_cli_photo_weight(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_dataset
    app = os.path.join(ROOT, "apps", "app_intrinsic3d")
    assert os.path.exists(app), "apps/app_intrinsic3d has not been built (run __graft_entry__.build())"
    sc = synthetic.make_scene(radius_vox=14, K=6, width=128, height=96, levels=1, seed=9, lum_noise=0.003, **BUMPY)    # test_gpu_track.py::test_cli_tracked_poses
    cam = track_twin.level_camera(sc["intr"], np.zeros(5), sc["width"], sc["height"], 0)
    for f, fr in enumerate(sc["frames"]):
        fr["depth"][0] = track_twin.raycast_scene(sc["scene"], cam, track_twin.ref_from_pose(sc["poses"][f]))[0]
    runs = {"absent": {}, "zero": dict(tracked_poses_photo_weight="0"), "photo": dict(tracked_poses_photo_weight="0.1")}
    out = {}
    for name, extra in runs.items():
        d = tmp_path / name
        s, i = make_dataset.write_dataset(str(d), sc, grid_levels=2, rgbd_levels=1, iterations=2, extra_frames=3, output_tracked_poses_prefix="./intrinsic3d/tracked", **extra)
        r = subprocess.run([app, "-s", s, "-i", i], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = r.stdout
    files = sorted(p.name for p in (tmp_path / "absent" / "intrinsic3d").iterdir() if p.is_file())
    assert "tracked_g0_p0.txt" in files and "tracked_g1_p0.txt" in files
    for name in files:                                    # key "0" is the key absent: every output byte
        assert (tmp_path / "absent" / "intrinsic3d" / name).read_bytes() == (tmp_path / "zero" / "intrinsic3d" / name).read_bytes(), name
    assert "photometric samples" not in out["absent"] and "photometric samples" not in out["zero"] and "photometric samples" in out["photo"]
    assert sorted(p.name for p in (tmp_path / "photo" / "intrinsic3d").iterdir() if p.is_file()) == files
    for name in ("poses_g1_p0.txt", "poses_g0_p0.txt"):   # the sensor's poses do not depend on the key
        assert (tmp_path / "absent" / "intrinsic3d" / name).read_bytes() == (tmp_path / "photo" / "intrinsic3d" / name).read_bytes(), name
    for post in ("g1_p0", "g0_p0"):
        tracked = np.loadtxt(tmp_path / "photo" / "intrinsic3d" / f"tracked_{post}.txt")
        poses = np.loadtxt(tmp_path / "photo" / "intrinsic3d" / f"poses_{post}.txt")
        assert tracked.shape == poses.shape == (9, 8)
        assert np.array_equal(tracked[:6], poses[:6])     # keyframes: their refined poses
        assert np.all(np.isfinite(tracked))
        for i in range(6, 9):                             # the extra frames repeat the last keyframe's image: a registered pose keeps its inliers, so it is within
            assert np.linalg.norm(tracked[i, 1:4] - poses[5, 1:4]) < 0.05      # the association gate (max_distance, 5 cm) of where it started
