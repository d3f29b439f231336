"""The scenes and volume utilities that the fusion tests share (test infrastructure, no tests in here): the orbit scene of the point-query tests, the textured
frames of the fusion tests, and the dense-box reading of a volume's state that the merge tests introduced.

Fixtures: a test module takes them by name (`from fusion_cases import fusion_frames, scenes  # noqa: F401`).  They are module-scoped, so each importing module
gets its own instance.  `scenes` asks for `fusion_frames`: a module that imports `scenes` imports `fusion_frames` with it.

The asserts in here are not rewritten by pytest: each carries its own message."""
import math
import os
import sys

import numpy as np
import pytest

import fusion_merge_twin as MT
import helpers
import query_cases as Q
import track_twin
from intrinsic3d_amd import binding as B, synthetic

# ---- the orbit scene: a sphere of 14 voxels seen by four 96 x 72 cameras 8 degrees apart ------------------------------------------------------------------
VS = Q.VS
W, H = 96, 72
FX = 525.0 * W / 640.0
INTR = np.array([FX, FX, (W - 1) * 0.5, (H - 1) * 0.5])
RADIUS_VOX = 14
BGR = np.full((H, W, 3), 128, np.uint8)


def fusion_scene():
    margin = int(np.ceil(RADIUS_VOX + 3.2 + 4))
    return synthetic.Scene(np.full(3, (margin + 2) * VS), RADIUS_VOX * VS, 0.5 * VS, 40.0)


def orbit_pose(scene, theta_deg, elev_deg=20.0):
    th, el = math.radians(theta_deg), math.radians(elev_deg)
    d = scene.R * FX / (0.35 * H)
    return synthetic.look_at_pose(scene.c + d * np.array([math.sin(th) * math.cos(el), math.sin(el), math.cos(th) * math.cos(el)]), scene.c)


def orbit_frames():
    """(scene, [(depth, pose)] of four noisy frames, query points): pure numpy"""
    scene = fusion_scene()
    cam = track_twin.level_camera(INTR, np.zeros(5), W, H, 0)
    rng = np.random.default_rng(2)
    frames = []
    for i in range(4):
        p = orbit_pose(scene, 8.0 * i)
        d = track_twin.raycast_scene(scene, cam, track_twin.ref_from_pose(p))[0]
        d[d > 0] += rng.normal(0.0, 0.0015, int((d > 0).sum())).astype(np.float32)
        frames.append((d, p))
    # points around the visible side of the sphere, +- 1.5 voxels off the surface, and a few far away
    look = np.array([math.sin(math.radians(12.0)), math.sin(math.radians(20.0)), math.cos(math.radians(12.0))])
    dirs = rng.normal(size=(6000, 3)) * 0.5 + look; dirs /= np.sqrt((dirs * dirs).sum(1, keepdims=True))
    dirs = dirs[dirs @ look > 0.75][:2000]
    pts = scene.c + dirs * (scene.R + rng.uniform(-1.5, 1.5, dirs.shape[0]) * VS)[:, None]
    pts = np.concatenate([pts, scene.c + rng.uniform(-3, 3, (50, 3)) * scene.R, [[np.nan, 0.0, 0.0]]])
    return scene, frames, pts


@pytest.fixture(scope="module")
def fusion_frames():
    return orbit_frames()


def fused(frames, query=None):
    """the orbit frames fused into a fresh volume (the caller closes it); with `query`, those points are queried before every frame"""
    f = B.Fusion(VS, 0.1, 10.0, initial_capacity=1 << 16)
    intr = INTR.astype(np.float32)
    for d, p in frames:
        if query is not None:
            f.query_points(query)
        f.integrate(d, intr, BGR, intr, helpers.c2w(p), 2)
    return f


# ---- the textured frames of the fusion tests ----------------------------------------------------------------------------------------------------------------
TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")                  # make_dataset lives there


def textured_frames(seed=9, K=6, radius=14, w=128, h=96, noise=0.0):
    """(scene dict, [(depth, bgr with three distinct channels, camera -> world)]) of synthetic.make_scene's keyframes"""
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    from make_dataset import pose_vec_to_cam_to_world
    sc = synthetic.make_scene(radius_vox=radius, K=K, width=w, height=h, levels=1, seed=seed)
    rng = np.random.default_rng(seed)
    out = []
    for fr, pose in zip(sc["frames"], sc["poses"]):
        d = fr["depth"][0].copy()
        if noise > 0:
            d[d > 0] += rng.normal(0, noise, int((d > 0).sum())).astype(np.float32)
        bgr = fr["bgr"][0].copy(); bgr[..., 0] = bgr[..., 0] // 2; bgr[..., 2] = 255 - bgr[..., 2] // 3          # three distinct channels
        out.append((d, bgr, pose_vec_to_cam_to_world(np.asarray(pose, np.float64)).astype(np.float32)))
    return sc, out


# ---- the state of a volume over a dense box of keys ---------------------------------------------------------------------------------------------------------
VS2 = 0.00390625                                    # 2^-8: m vs / vs is exact for every lattice translation m
FIELDS = ("sdf", "weight", "color", "first_frame")
COUNTS = ("ordinal", "source_voxels", "sampled", "allocated", "aligned")
AXIS = np.array([0.3, -0.8, 0.52])
POSE = np.concatenate([AXIS / np.linalg.norm(AXIS) * math.radians(20.0), [0.0131, -0.0207, 0.0049]])     # oblique, about 20 degrees, no lattice translation


def dense(lo, hi):
    return np.ascontiguousarray(np.stack(np.meshgrid(*[np.arange(lo[a], hi[a], dtype=np.int32) for a in range(3)], indexing="ij"), -1).reshape(-1, 3))


def fuse(frames, vs, capacity=1 << 16):
    f = B.Fusion(vs, 0.1, 10.0, initial_capacity=capacity)
    for d, intr, bgr, T, er in frames:
        f.integrate(d, intr, bgr, intr, T, er)
    return f


def snapshot(f, box):
    """every stored voxel of f inside the box, as the twin's volume"""
    dv = f.debug_voxels(box); s = dv["found"]
    return MT.volume(box[s], dv["sdf"][s], dv["weight"][s], dv["color"][s], dv["first_frame"][s])


def moved_box(lo, hi, R, tv):
    """a box that holds the image of [lo, hi) under a = R k + tv, and [lo, hi) itself"""
    c = np.array([[(lo, hi)[(i >> a) & 1][a] for a in range(3)] for i in range(8)], np.float64) @ np.asarray(R).T + tv
    return np.minimum(lo, np.floor(c.min(0)).astype(np.int64) - 3), np.maximum(hi, np.ceil(c.max(0)).astype(np.int64) + 4)


def same_render(a, c):
    assert a["stats"] == c["stats"], ("stats", a["stats"], c["stats"])
    for k in ("depth", "normal"):
        assert np.array_equal(a[k], c[k]), (k, int((a[k] != c[k]).sum()))


class Scene:
    def __init__(self, frames, vs):
        self.frames, self.vs = frames, vs
        with fuse(frames, vs) as f:                                              # a finished copy: how many voxels there are, and where
            f.finish(0); ex = f.export(); allocated = f.info()["allocated"]
        self.lo = ex["keys"].min(0).astype(np.int64) - 12; self.hi = ex["keys"].max(0).astype(np.int64) + 13
        self.box = dense(self.lo, self.hi)
        with fuse(frames, vs) as f:
            inside = len(snapshot(f, self.box)["keys"])
            assert inside == allocated, ("stored voxels inside the box", inside, "allocated", allocated)   # the box holds every stored voxel, the weightless ones included

    def a(self, capacity=1 << 16):
        return fuse(self.frames[:2], self.vs, capacity)

    def b(self):
        return fuse(self.frames[2:3], self.vs)


@pytest.fixture(scope="module")
def scenes(fusion_frames):
    _, frames, _ = fusion_frames
    intr = INTR.astype(np.float32)
    over = [(d, intr, BGR, helpers.c2w(p), 2) for d, p in frames]
    sc, fr = textured_frames(seed=5, K=3, radius=10, w=96, h=72)
    ti = sc["intr"].astype(np.float32)
    return dict(overlapping=Scene(over, VS), textured=Scene([(d, ti, bgr, T, 2) for d, bgr, T in fr], float(sc["voxel_size"])), pow2=Scene(over, VS2))
