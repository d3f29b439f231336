"""The scenes of the tracking tests (test infrastructure, no tests in here): the bumpy sphere with keyframes that i3d_track_frame registers on, the same sphere
without bumps that only colour can register, the contexts over them, and the model ray-cast through the renderer.

The asserts in here are not rewritten by pytest: each carries its own message."""
import numpy as np
import pytest

import helpers
import track_rgbd_twin as rgbd_twin
import track_twin
from intrinsic3d_amd import binding, synthetic

DIST = helpers.TRACK_DIST
BUMPY = dict(bump_amp_vox=3.0, bump_freq=60.0)          # the default bumps (half a voxel) leave rotation about the sphere's centre almost free
SHIFT = (-100000, -99987, -100021)                      # the negative octant, far from the origin
CASES = {"plain": dict(), "distortion": dict(dist=DIST), "negative_octant": dict(shift=SHIFT)}


def scene(shift=None, seed=5):
    sc = dict(helpers.small_scene(seed=seed, radius_vox=16, K=3, width=160, height=120, levels=1, **BUMPY))
    vs = float(sc["voxel_size"])
    sc["albedo_true"] = sc["scene"].albedo(sc["keys"].astype(np.float64) * vs)
    # a camera that is not a keyframe
    eye = sc["center"] + 3.1 * sc["scene"].R * np.array([0.35, 0.45, -0.82]) / np.linalg.norm([0.35, 0.45, -0.82])
    sc["truth"] = synthetic.look_at_pose(eye, sc["center"])
    if shift is not None:                            # the same scene far from the origin (world shifted by t: tr' = tr - R t)
        shift = np.asarray(shift, np.int64)
        sc["keys"] = (sc["keys"] + shift[None, :]).astype(np.int32)
        t = shift.astype(np.float64) * vs
        poses = np.array(sc["poses"], np.float64)
        for f in range(len(poses)):
            poses[f, 3:] = poses[f, 3:] - synthetic.aa_to_rotmat(poses[f, :3]) @ t
        sc["poses"] = poses
        tr = np.array(sc["truth"], np.float64); tr[3:] = tr[3:] - synthetic.aa_to_rotmat(tr[:3]) @ t
        sc["truth"] = tr
    return sc


def context(sc, dist=None, sdf_refined=None):
    ctx = binding.Context(0)
    ctx.set_grid(sc["voxel_size"], sc["keys"], sc["sdf"], sc["sdf"] if sdf_refined is None else sdf_refined, sc["albedo_true"], sc["weight"], sc["color"])
    ctx.set_frames(sc["frames"], sc["levels"])
    ctx.set_camera(sc["intr"], np.zeros(5) if dist is None else dist, sc["poses"])
    return ctx


def view(ctx, sc, pose, level=0, dist=None):
    """the model ray-cast through the renderer: (depth, world normal) of the level's camera"""
    cam = track_twin.level_camera(sc["intr"], np.zeros(5) if dist is None else dist, sc["width"], sc["height"], level)
    out = ctx.render_view(frame=-1, planes=("depth", "normal"), camera=dict(width=cam["w"], height=cam["h"], intr=cam["intr"], dist=cam["dist"], pose=pose))
    return out["depth"], out["normal"]


def rc(fn):
    """the status code of the I3DError that fn must raise"""
    with pytest.raises(binding.I3DError) as e:
        fn()
    return int(str(e.value).split("failed (")[1].split(")")[0])


def centre_in_camera(scene, a, b, vs):
    """distance between the images of the sphere's centre under two world -> camera poses, voxels"""
    q = [synthetic.aa_to_rotmat(np.asarray(p[:3], np.float64)) @ scene.c + np.asarray(p[3:], np.float64) for p in (a, b)]
    return float(np.linalg.norm(q[0] - q[1])) / vs


# ---- the photometric trackers: the true albedo in the grid, the scene's SH at every voxel -------------------------------------------------------------------
# The frames of these tests are the model cast at the true pose, so at the truth every frame pixel projects onto a pixel centre of the cast: a corner of the
# bilinear cells, where the interpolant's derivative jumps.  Steps below about 1e-5 rad / 1e-5 m then wander instead of shrinking, so the stop rule is 1e-5 (the
# bars are 3.5e-4 rad and 2e-4 m) and the budget 60 iterations.
DESC = dict(iterations=[60], stop_rotation=1e-5, stop_translation=1e-5)
WEIGHTS = dict(geometric_weight=1.0, photo_weight=0.1)
BAR_DEG, BAR_VOX = 0.02, 0.05                          # test_gpu_track.py::test_converges_to_the_true_pose


def smooth_scene(seed=5):
    """scene() without bumps: a sphere, whose depth is blind to any rotation about its centre"""
    sc = dict(helpers.small_scene(seed=seed, radius_vox=16, K=3, width=160, height=120, levels=1, bump_amp_vox=0.0))
    vs = float(sc["voxel_size"])
    sc["albedo_true"] = sc["scene"].albedo(sc["keys"].astype(np.float64) * vs)
    eye = sc["center"] + 3.1 * sc["scene"].R * np.array([0.35, 0.45, -0.82]) / np.linalg.norm([0.35, 0.45, -0.82])
    sc["truth"] = synthetic.look_at_pose(eye, sc["center"])
    return sc


def voxel_sh(sc):
    return np.tile(synthetic.SH_TRUE, (sc["keys"].shape[0], 1))


def smooth_starts(sc):
    rng = np.random.default_rng(17)
    return [rgbd_twin.orbit(sc["truth"], sc["center"], rng, 2.0, 3.0 * float(sc["voxel_size"])) for _ in range(3)]


def rgbd_context(sc, dist=None, sh=True):
    ctx = context(sc, dist)
    if sh:
        ctx.set_voxel_sh(voxel_sh(sc))
    return ctx
