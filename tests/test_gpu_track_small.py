"""The association pass of i3d_track_frame / i3d_track_frame_rgbd on frames of a few hundred pixels, where its last workgroup is partial: 20 x 12 is one workgroup
of 240 lanes in use, 33 x 17 (odd width) is two full workgroups and a tail of 49.  The 160 x 120 frames of test_gpu_track.py are exactly 75 workgroups.  The
frame brings its own camera (use_context_camera = 0), distorted, with a focal length at which the sphere of test_gpu_track.py fills the image; the sums are held
to their numpy statements by the rule of test_sums_match_twin, and the (1, 0) rgbd sums to the depth-only ones byte for byte."""
import math

import numpy as np
import pytest

import track_rgbd_twin as rgbd_twin
import track_twin
from intrinsic3d_amd import synthetic
from track_cases import BUMPY, DIST, rgbd_context, scene

pytestmark = pytest.mark.gpu

SIZES = {"20x12": (20, 12), "33x17": (33, 17)}
MIN_COUNT = 64                                        # TRACK_MIN_INLIERS: below it the solve reports status 2
SEED = 3                                              # of the two perturbed poses, as test_sums_match_twin


def _fill_camera(sc, w, h):
    """the camera of a w x h frame at the truth pose whose corner rays still meet the sphere at its deepest bump"""
    scene = sc["scene"]
    Rt = synthetic.aa_to_rotmat(np.asarray(sc["truth"][:3], np.float64))
    eye = -Rt.T @ np.asarray(sc["truth"][3:], np.float64)
    d = float(np.linalg.norm(eye - sc["center"]))
    inner = scene.R - BUMPY["bump_amp_vox"] * float(sc["voxel_size"])
    half_diag = math.hypot(0.5 * (w - 1), 0.5 * (h - 1))
    f = 1.2 * half_diag / math.tan(math.asin(inner / d))
    return track_twin.level_camera(np.array([f, f, 0.5 * (w - 1), 0.5 * (h - 1)]), DIST, w, h, 0)


@pytest.fixture(scope="module")
def model():
    sc = scene()
    ctx = rgbd_context(sc)
    yield sc, ctx
    ctx.close()


@pytest.fixture(scope="module", params=list(SIZES))
def small(request, model):
    """the frame, the two poses, the model planes cast at the reference pose and the twins' sums of one size"""
    sc, ctx = model
    w, h = SIZES[request.param]
    cam = _fill_camera(sc, w, h)
    vs = float(sc["voxel_size"])

    def view(pose):
        out = ctx.render_view(frame=-1, planes=("depth", "normal", "intensity"), camera=dict(width=w, height=h, intr=cam["intr"], dist=cam["dist"], pose=pose))
        return out["depth"], out["normal"], out["intensity"]

    depth, _, lum = view(sc["truth"])
    assert (depth > 0).sum() > 0.9 * depth.size, "the sphere does not fill the frame"
    rng = np.random.default_rng(SEED)
    pose_ref = track_twin.perturb(sc["truth"], rng, 0.7, 1.5 * vs)
    pose_cur = track_twin.perturb(sc["truth"], rng, 0.5, 1.0 * vs)
    md, mn, mi = view(pose_ref)
    vtx, nrm = track_twin.frame_points(depth, cam)
    Rc, tc = track_twin.pose_to_cw(pose_cur)
    ref = track_twin.ref_from_pose(pose_ref)
    tw = track_twin.associate(vtx, nrm, md, mn, cam, ref, Rc, tc, 0.05, 0.8)
    tw_rgbd = rgbd_twin.associate_rgbd(vtx, nrm, md, mn, mi, lum, cam, ref, Rc, tc, 0.05, 0.8, 1.0, 0.1)
    kw = dict(levels=1, intr=cam["intr"], dist=cam["dist"])
    return dict(ctx=ctx, cam=cam, depth=depth, lum=lum, pose_ref=pose_ref, pose_cur=pose_cur, tw=tw, tw_rgbd=tw_rgbd, kw=kw)


def test_small_sums_match_twin(small):
    s, tw, cam = small, small["tw"], small["cam"]
    sums, n = s["ctx"].debug_track_sums(s["depth"], 0, s["pose_ref"], s["pose_cur"], **s["kw"])
    print(cam["w"], cam["h"], "inliers", n, tw["inliers"], "max rel", np.max(np.abs(sums - tw["sums"]) / np.maximum(tw["abs_sums"], 1e-300)))
    assert tw["inliers"] >= MIN_COUNT                                       # the comparison is not one of empty sums
    flips = abs(n - tw["inliers"])
    assert flips <= 0.001 * cam["w"] * cam["h"], (n, tw["inliers"])          # < 1 at these sizes: no flip
    assert sums[28] == n
    assert np.all(np.abs(sums - tw["sums"]) <= 1e-9 * tw["abs_sums"]), np.max(np.abs(sums - tw["sums"]) / tw["abs_sums"])


def test_small_rgbd_sums_match_twin(small):
    s, tw, cam = small, small["tw_rgbd"], small["cam"]
    sums, n, m = s["ctx"].debug_track_rgbd_sums(s["depth"], s["lum"], 0, s["pose_ref"], s["pose_cur"], geometric_weight=1.0, photo_weight=0.1, **s["kw"])
    print(cam["w"], cam["h"], "inliers", n, tw["inliers"], "samples", m, tw["samples"], "max rel", np.max(np.abs(sums - tw["sums"]) / np.maximum(tw["abs_sums"], 1e-300)))
    assert tw["inliers"] >= MIN_COUNT and tw["samples"] >= MIN_COUNT
    flips = abs(n - tw["inliers"]) + abs(m - tw["samples"])
    assert flips <= 0.001 * cam["w"] * cam["h"], (n, tw["inliers"], m, tw["samples"])
    assert sums[28] == n and sums[30] == m
    assert np.all(np.abs(sums - tw["sums"]) <= 1e-9 * tw["abs_sums"]), np.max(np.abs(sums - tw["sums"]) / np.maximum(tw["abs_sums"], 1e-300))


def test_small_rgbd_reduces_to_the_depth_only_sums(small):
    s = small
    old, n_old = s["ctx"].debug_track_sums(s["depth"], 0, s["pose_ref"], s["pose_cur"], **s["kw"])
    new, n_new, m = s["ctx"].debug_track_rgbd_sums(s["depth"], s["lum"], 0, s["pose_ref"], s["pose_cur"], geometric_weight=1.0, photo_weight=0.0, **s["kw"])
    assert n_old >= MIN_COUNT
    assert n_old == n_new and m == 0 and old.tobytes() == new[:29].tobytes() and new[29] == 0.0 and new[30] == 0.0
