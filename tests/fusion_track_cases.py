"""The scene of the fusion tracking tests (test infrastructure, no tests in here): a bumpy sphere of 20 voxels seen at 160 x 120 from an arc around it, and the
volume fused from six noisy frames of that arc.  test_gpu_fusion_track.py tests i3d_fusion_render / i3d_fusion_track on it; the "fusion" case of
track_loop_cases.py is this scene."""
import math

import numpy as np

import helpers
import track_cases
import track_twin
from intrinsic3d_amd import binding as B, synthetic

VS = 0.004
W, H = 160, 120
FX = 525.0 * W / 640.0
INTR = np.array([FX, FX, (W - 1) * 0.5, (H - 1) * 0.5])
INTR32 = INTR.astype(np.float32)
RADIUS_VOX = 20
BUMPY = track_cases.BUMPY                               # the bumps pin rotation about the sphere's centre
BGR = np.full((H, W, 3), 128, np.uint8)


def scene(shift=None):
    margin = int(np.ceil(RADIUS_VOX + 3.2 + 4))
    c = np.full(3, (margin + 2) * VS)
    if shift is not None:
        c = c + np.asarray(shift, np.float64) * VS
    return synthetic.Scene(c, RADIUS_VOX * VS, BUMPY["bump_amp_vox"] * VS, BUMPY["bump_freq"])


def cam_dist(scene):
    return scene.R * FX / (0.35 * H)


def arc_pose(scene, theta_deg, elev_deg=20.0, scale=1.0):
    th, el = math.radians(theta_deg), math.radians(elev_deg)
    eye = scene.c + scale * cam_dist(scene) * np.array([math.sin(th) * math.cos(el), math.sin(el), math.cos(th) * math.cos(el)])
    return synthetic.look_at_pose(eye, scene.c)


def depth(scene, pose, noise=0.0, rng=None):
    cam = track_twin.level_camera(INTR, np.zeros(5), W, H, 0)
    d = track_twin.raycast_scene(scene, cam, track_twin.ref_from_pose(pose))[0]
    if noise > 0:
        d[d > 0] += rng.normal(0.0, noise, int((d > 0).sum())).astype(np.float32)
    return d


def integrate(f, depth, pose):
    f.integrate(depth, INTR32, BGR, INTR32, helpers.c2w(pose), 2)


def fused(scene, n=6, seed=2, correct=None, cap=1 << 16):
    """n noisy frames of the arc, 6 degrees apart, fused into a fresh volume (the caller closes it)"""
    rng = np.random.default_rng(seed)
    f = B.Fusion(VS, 0.1, 10.0, initial_capacity=cap)
    for i in range(n):
        p = arc_pose(scene, 6.0 * i)
        integrate(f, depth(scene, p, 0.0015, rng), p)
    return f
