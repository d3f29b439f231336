"""i3d_fusion_render / i3d_fusion_track: the fusion volume as a model while it is being fused.  The cast of the table equals the context's cast
of the exported volume bit for bit, the cached bitmap follows integrate and table growth, tracking equals the context's tracking, neither changes the fusion, drift
of the input poses is removed, and app_fusion's opt-in keys."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import fusion_track_cases as FT
import helpers
import track_twin
from fusion_track_cases import BGR, FX, H, INTR, VS, W
from helpers import TRACK_DIST as DIST
from intrinsic3d_amd import binding as B, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

# Bars of the drift tests: 0.5 voxel on the camera centre, 0.5 degree on the orientation.  Measured on an MI355X: centre <= 0.19 voxel, orientation 0.2 - 0.33
# degree — the weakly pinned rotation about the sphere's centre (min_pivot_ratio ~1e-3), which moves this 20-voxel surface by ~0.02 voxel
ROT_BAR_DEG = 0.5


def _cameras(scene):
    d = FT.cam_dist(scene)
    return [dict(width=W, height=H, intr=INTR, pose=FT.arc_pose(scene, 17.0, 31.0)),
            dict(width=W, height=H, intr=INTR, dist=DIST, pose=FT.arc_pose(scene, 8.0, 12.0, 1.1)),
            dict(width=W, height=H, intr=INTR, pose=FT.arc_pose(scene, 25.0, 18.0), depth_range=(d - 0.5 * scene.R, d - 0.2 * scene.R))]


def _cast(obj, cam, fusion):
    kw = dict(camera={k: v for k, v in cam.items() if k != "depth_range"}, depth_range=cam.get("depth_range"))
    if fusion:
        return obj.render(planes=("depth", "normal"), **kw)
    return obj.render_view(frame=-1, refined=False, planes=("depth", "normal"), **kw)


def _same_cast(a, b):
    assert np.array_equal(a["depth"], b["depth"]) and np.array_equal(a["normal"], b["normal"])
    assert a["stats"]["hits"] == b["stats"]["hits"] and a["stats"]["samples"] == b["stats"]["samples"]


@pytest.mark.parametrize("shift", [None, (-100000, -99987, -100021)], ids=["plain", "negative_octant"])
def test_fusion_cast_equals_context_cast(shift):
    scene = FT.scene(shift)
    cams = _cameras(scene)
    f = FT.fused(scene)
    try:
        before = [_cast(f, c, True) for c in cams]
        assert before[0]["stats"]["hits"] > 0.2 * W * H
        assert 0 < before[2]["stats"]["hits"] < before[0]["stats"]["hits"]          # the depth range clips the sphere
        f.finish(0)
        ctx = helpers.context_of_fusion(f, VS)
        try:
            for c, a in zip(cams, before):
                _same_cast(a, _cast(ctx, c, False))
                _same_cast(a, _cast(f, c, True))                                     # finish(0) leaves the table as it was
        finally:
            ctx.close()
    finally:
        f.close()
    if shift is None:                                                                # the table as finish(10) left it equals its own export
        f = FT.fused(scene)
        try:
            f.finish(10)
            ctx = helpers.context_of_fusion(f, VS)
            try:
                for c in cams:
                    _same_cast(_cast(f, c, True), _cast(ctx, c, False))
            finally:
                ctx.close()
        finally:
            f.close()


def test_cache_follows_integrate_and_growth():
    scene = FT.scene()
    rng = np.random.default_rng(4)
    poses = [FT.arc_pose(scene, 45.0 * i) for i in range(8)]                          # every frame sees new surface: the table keeps growing
    frames = [FT.depth(scene, p, 0.0015, rng) for p in poses]
    caps = []
    with B.Fusion(VS, 0.1, 10.0, initial_capacity=1 << 10) as probe:
        for d, p in zip(frames, poses):
            FT.integrate(probe, d, p)
            caps.append(probe.info()["capacity"])
    grew = [i for i in range(1, len(caps)) if caps[i] > caps[i - 1]]
    assert grew, caps
    k = grew[-1]                                                                     # integrating frame k grows the table
    cam = _cameras(scene)[0]
    with B.Fusion(VS, 0.1, 10.0, initial_capacity=1 << 10) as a, B.Fusion(VS, 0.1, 10.0, initial_capacity=1 << 10) as b:
        for d, p in zip(frames[:k], poses[:k]):
            FT.integrate(a, d, p)
        first = _cast(a, cam, True)
        cap = a.info()["capacity"]
        FT.integrate(a, frames[k], poses[k])
        assert a.info()["capacity"] > cap
        second = _cast(a, cam, True)
        for d, p in zip(frames[:k + 1], poses[:k + 1]):
            FT.integrate(b, d, p)
        ref = _cast(b, cam, True)
    _same_cast(second, ref)
    assert not np.array_equal(first["depth"], second["depth"])


def test_fusion_track_equals_context_track():
    scene = FT.scene()
    f = FT.fused(scene)
    try:
        truth = FT.arc_pose(scene, 14.0, 24.0)
        depth = FT.depth(scene, truth)
        start = track_twin.perturb(truth, np.random.default_rng(21), 1.0, 3.0 * VS)
        f.finish(0)
        a_pose, a_st = f.track(depth, start, INTR)
        ctx = helpers.context_of_fusion(f, VS)
        try:
            b_pose, b_st = ctx.track_frame(depth, start, intr=INTR, refined=False)
        finally:
            ctx.close()
    finally:
        f.close()
    assert np.array_equal(a_pose, b_pose) and a_st == b_st
    assert a_st["status"] == 0 and track_twin.rot_err_deg(a_pose, truth) < 0.1 and track_twin.centre_err(a_pose, truth) < 0.5 * VS, a_st


def test_render_and_track_change_nothing():
    scene = FT.scene()
    rng = np.random.default_rng(6)
    poses = [FT.arc_pose(scene, 6.0 * i) for i in range(5)]
    frames = [FT.depth(scene, p, 0.0015, rng) for p in poses]
    cam = _cameras(scene)[0]
    out = []
    for probe in (False, True):
        with B.Fusion(VS, 0.1, 10.0, initial_capacity=1 << 12) as f:
            for d, p in zip(frames, poses):
                if probe:
                    f.render(camera=cam, planes=("depth", "normal"))
                    f.track(d, track_twin.perturb(p, np.random.default_rng(1), 0.5, VS), INTR)
                FT.integrate(f, d, p)
            f.finish(10)
            out.append(f.export())
    for k in ("keys", "sdf", "weight", "color"):
        assert np.array_equal(out[0][k], out[1][k]), k


def _walk(n, seed=13):
    """input pose perturbations: a seeded random walk with drift of the camera (rotation about a drifting axis, centre offset), zero at frame 0"""
    rng = np.random.default_rng(seed)
    ax0 = rng.normal(size=3); ax0 /= np.linalg.norm(ax0)
    dir0 = rng.normal(size=3); dir0 /= np.linalg.norm(dir0)
    Rw, cw = [np.eye(3)], [np.zeros(3)]
    for _ in range(1, n):
        w = math.radians(0.07) * ax0 + rng.normal(0.0, math.radians(0.04), 3)
        Rw.append(synthetic.aa_to_rotmat(w) @ Rw[-1])
        cw.append(cw[-1] + 0.25 * VS * dir0 + rng.normal(0.0, 0.15 * VS, 3))
    return Rw, cw


def _apply(pose, Rw, cw):
    R = synthetic.aa_to_rotmat(pose[:3]); c = -R.T @ pose[3:]
    R2 = Rw @ R; c2 = c + cw
    return np.concatenate([synthetic.rotmat_to_aa(R2), -R2 @ c2])


def _mat(pose):
    M = np.eye(4); M[:3, :3] = synthetic.aa_to_rotmat(pose[:3]); M[:3, 3] = pose[3:]
    return M


def _vec(M):
    return np.concatenate([synthetic.rotmat_to_aa(M[:3, :3]), M[:3, 3]])


def _drift_sequence(n=24):
    scene = FT.scene()
    truth = [FT.arc_pose(scene, 60.0 * i / (n - 1)) for i in range(n)]
    Rw, cw = _walk(n)
    given = [np.asarray(truth[0], np.float64)] + [_apply(p, r, c) for p, r, c in zip(truth[1:], Rw[1:], cw[1:])]
    rng = np.random.default_rng(3)
    frames = [FT.depth(scene, p, 0.0005, rng) for p in truth]
    return scene, truth, given, frames


def _held_out(scene):
    return dict(width=W, height=H, intr=INTR, pose=FT.arc_pose(scene, 30.0, 35.0))


def _median_gap(a, b):
    m = (a["depth"] > 0) & (b["depth"] > 0)
    assert m.sum() > 0.2 * W * H
    return float(np.median(np.abs(a["depth"][m] - b["depth"][m])))


def test_drift_is_removed():
    scene, truth, given, frames = _drift_sequence()
    assert track_twin.rot_err_deg(given[-1], truth[-1]) >= 1.0 and track_twin.centre_err(given[-1], truth[-1]) >= 3.0 * VS
    assert np.array_equal(given[0], truth[0])
    vols = {}
    tracked = []
    for mode in ("true", "given", "tracked"):
        f = B.Fusion(VS, 0.1, 10.0, initial_capacity=1 << 16)
        vols[mode] = f
        for i, d in enumerate(frames):
            pose = truth[i] if mode == "true" else given[i]
            if mode == "tracked" and i > 0:
                guess = _vec(_mat(given[i]) @ np.linalg.inv(_mat(given[i - 1])) @ _mat(tracked[-1]))
                p, st = f.track(d, guess, INTR)
                pose = p if st["status"] in (0, 1) else guess
            if mode == "tracked":
                tracked.append(np.asarray(pose, np.float64))
            FT.integrate(f, d, pose)
    try:
        rot = [track_twin.rot_err_deg(p, t) for p, t in zip(tracked, truth)]
        cen = [track_twin.centre_err(p, t) / VS for p, t in zip(tracked, truth)]
        assert max(rot) < ROT_BAR_DEG and max(cen) < 0.5, (max(rot), max(cen))
        cam = _held_out(scene)
        ref = _cast(vols["true"], cam, True)
        gap_tracked = _median_gap(_cast(vols["tracked"], cam, True), ref)
        gap_given = _median_gap(_cast(vols["given"], cam, True), ref)
        assert gap_tracked * 5.0 <= gap_given, (gap_tracked, gap_given)
    finally:
        for f in vols.values():
            f.close()


def _msg(fn):
    with pytest.raises(B.I3DError) as e:
        fn()
    s = str(e.value)
    return int(s.split("failed (")[1].split(")")[0]), s


def test_empty_volume_and_errors():
    scene = FT.scene()
    truth = FT.arc_pose(scene, 10.0)
    depth = FT.depth(scene, truth)
    with B.Fusion(VS, 0.1, 10.0) as f:
        pose, st = f.track(depth, truth, INTR)
        assert st["status"] == 2 and np.array_equal(pose, np.asarray(truth, np.float64))
        out = f.render(camera=dict(width=W, height=H, intr=INTR, pose=truth))
        assert out["stats"]["hits"] == 0 and not out["depth"].any()
        FT.integrate(f, depth, truth)
        L = f.L
        assert L.i3d_fusion_render(None, B.RenderDesc(), None, None, None) == 1
        assert L.i3d_fusion_track(None, B.track_desc_default(intr=INTR), W, H, B._p(depth), None, None) == 1
        assert L.i3d_fusion_render(f.h, None, None, None, None) == 1 and "descriptor" in L.i3d_fusion_last_error(f.h).decode()
        d = B.RenderDesc(); d.frame = 0; d.width, d.height = W, H
        assert L.i3d_fusion_render(f.h, d, None, None, None) == 1 and "frame" in L.i3d_fusion_last_error(f.h).decode()
        td = B.track_desc_default(intr=INTR)
        p = np.array(truth, np.float64)
        assert L.i3d_fusion_track(f.h, None, W, H, B._p(depth), B._p(p), None) == 1 and "descriptor" in L.i3d_fusion_last_error(f.h).decode()
        assert L.i3d_fusion_track(f.h, td, W, H, None, B._p(p), None) == 1 and "depth" in L.i3d_fusion_last_error(f.h).decode()
        assert L.i3d_fusion_track(f.h, td, W, H, B._p(depth), None, None) == 1 and "pose" in L.i3d_fusion_last_error(f.h).decode()
        td.use_context_camera = 1
        assert L.i3d_fusion_track(f.h, td, W, H, B._p(depth), B._p(p), None) == 1 and "use_context_camera" in L.i3d_fusion_last_error(f.h).decode()
        cam = dict(width=W, height=H, intr=INTR, pose=truth)
        for bad, word in ((dict(width=0), "image size"), (dict(height=40000), "image size")):
            rc, m = _msg(lambda: f.render(camera={**cam, **bad}))
            assert rc == 1 and word in m, m
        for bad, word in ((dict(levels=0), "levels"), (dict(levels=5), "levels"), (dict(iterations=[101]), "iterations"), (dict(max_distance=0.0), "max_distance")):
            rc, m = _msg(lambda: f.track(depth, truth, INTR, **bad))
            assert rc == 1 and word in m, (bad, m)
        rc, m = _msg(lambda: f.track(depth, truth, [0.0, FX, INTR[2], INTR[3]]))
        assert rc == 1 and "focal" in m, m
        rc, m = _msg(lambda: f.track(depth[:12, :12], truth, INTR, levels=3))
        assert rc == 1 and "too small" in m, m
        rc, m = _msg(lambda: f.track(np.zeros((0, 4), np.float32), truth, INTR))
        assert rc == 1 and "image size" in m, m


def _tum_to_pose(row):
    """timestamp tx ty tz qx qy qz qw (camera -> world) -> world -> camera angle-axis | t"""
    t = row[1:4]; qx, qy, qz, qw = row[4:8]
    R = np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
                  [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
                  [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    Rw = R.T
    return np.concatenate([synthetic.rotmat_to_aa(Rw), -Rw @ t])


def test_cli_tracking(tmp_path):
    import make_dataset
    app = os.path.join(ROOT, "apps", "app_fusion")
    assert os.path.exists(app), "apps/app_fusion has not been built (run __graft_entry__.build())"
    scene, truth, given, frames = _drift_sequence()
    keys = np.zeros((1, 3), np.int32)
    sc = dict(voxel_size=VS, intr=INTR, keys=keys, sdf=np.zeros(1, np.float32), weight=np.ones(1, np.float32), color=np.zeros((1, 3), np.uint8),
              frames=[dict(depth=[d], bgr=[BGR]) for d in frames], poses=given)
    runs = {}
    for name, extra in (("plain", ""), ("tracked", 'track_frames: "1"\noutput_tracked_poses: "./fusion/tracked.txt"\n')):
        out = tmp_path / name
        s, _ = make_dataset.write_dataset(str(out), sc)
        with open(out / "fusion.yml", "a") as fh:
            fh.write(extra)
        r = subprocess.run([app, "-s", s, "-f", str(out / "fusion.yml")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[name] = (out, r.stdout)
    plain, tracked = runs["plain"][0], runs["tracked"][0]
    assert not (plain / "fusion" / "tracked.txt").exists()
    assert "tracking frame" in runs["tracked"][1] and "tracking frame" not in runs["plain"][1]
    traj = helpers.read_tum(tracked / "fusion" / "tracked.txt")
    assert traj.shape[1] == 8
    assert traj.shape[0] == len(frames)
    poses = [_tum_to_pose(r) for r in traj]
    rot = [track_twin.rot_err_deg(p, t) for p, t in zip(poses, truth)]
    cen = [track_twin.centre_err(p, t) / VS for p, t in zip(poses, truth)]
    assert max(rot) < ROT_BAR_DEG and max(cen) < 0.5, (max(rot), max(cen))
    tsdf = f"volume_{VS:g}.tsdf"
    a, b = B.tsdf_read(str(plain / "fusion" / tsdf)), B.tsdf_read(str(tracked / "fusion" / tsdf))
    assert a["keys"].shape != b["keys"].shape or not np.array_equal(a["sdf"], b["sdf"])
