"""The fault table of the entry points that read the stored field of a context or a fusion volume (render, ray-cast tracking, point queries, point-set
registration, depth frames on the field), pinned completely: for every call that validation must refuse, the return code, the whole text of
i3d_last_error / i3d_fusion_last_error, and that no output was written.  The expected values are tests/golden/model_errors.json, recorded once
(`python tests/test_gpu_model_errors.py --record [path]`) with the library as it stood before the host layer behind these entry points became one model view
(DESIGN.md section 33); they never come from the code under test.  Every call is refused in validation and no case launches a kernel that fails (the ray-cast
trackers build the model's cached brick bitmap before they look at the focal lengths, as they always did).

Handles: an empty context; the grid "plain" of register_cases without a camera, then with keyframes (4 x 4, one level), then with a camera, never with SH; a
fusion volume with one frame of test_gpu_query's."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fault_table import Outs, compare_with_golden, record_golden  # noqa: E402
import fusion_cases as FC  # noqa: E402  (the fusion frame of the point-query tests: the same scene, camera and size)
import register_cases as RC  # noqa: E402
import track_twin  # noqa: E402
from intrinsic3d_amd import binding as B  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "model_errors.json")
NAN, INF = float("nan"), float("inf")
INTR = [30.0, 30.0, 1.5, 1.5]
p = B._p


DEP = np.zeros((4, 4), np.float32)
LUM = np.zeros((4, 4), np.float32)
DEP2 = np.zeros((2, 4, 4), np.float32)
LUM2 = np.zeros((2, 4, 4), np.float32)
PTS = np.zeros((1, 3))
PIVOT = np.zeros(3)
NAN_POSE = [0.0, 0.0, 0.0, NAN, 0.0, 0.0]
INF_POSE = [INF, 0.0, 0.0, 0.0, 0.0, 0.0]
CAM = dict(width=4, height=4, intr=INTR, dist=np.zeros(5), pose=np.zeros(6))


def _render_cases(L):
    """i3d_render_view / i3d_fusion_render"""
    def ctx(d, planes=("depth",)):
        return lambda h, o: L.i3d_render_view(h, d, *[p(o.arr((4, 4, 3) if k == "normal" else (4, 4))) if k in planes else None for k in B.RENDER_PLANES],
                                              o.stats(B.RenderStats))

    def vol(d):
        return lambda h, o: L.i3d_fusion_render(h, d, p(o.arr((4, 4))), p(o.arr((4, 4, 3))), o.stats(B.RenderStats))
    free = lambda **kw: B._render_desc(dict(CAM, **kw), None)
    key = lambda frame, level=0: B._render_desc(None, None, frame, level)
    return [("render/context/null_descriptor", "grid", ctx(None)),
            ("render/context/no_grid", "empty", ctx(free())),
            ("render/context/no_grid_before_no_keyframes", "empty", ctx(key(0))),
            ("render/context/no_keyframes", "grid", ctx(key(0))),
            ("render/context/no_camera", "framed", ctx(key(0))),
            ("render/context/frame_out_of_range", "keyed", ctx(key(2))),
            ("render/context/level_out_of_range", "keyed", ctx(key(0, 1))),
            ("render/context/level_negative", "keyed", ctx(key(1, -1))),
            ("render/context/residual_without_keyframe", "grid", ctx(free(), ("depth", "residual"))),
            ("render/context/residual_before_size", "grid", ctx(free(width=0), ("residual",))),
            ("render/context/width_0", "grid", ctx(free(width=0))),
            ("render/context/height_too_large", "grid", ctx(free(height=32769))),
            ("render/context/shading_without_sh", "grid", ctx(free(), ("shading",))),
            ("render/context/keyframe_intensity_without_sh", "keyed", ctx(key(1), ("depth", "intensity"))),
            ("render/context/size_before_sh", "grid", ctx(free(height=-1), ("intensity",))),
            ("render/volume/null_descriptor", "volume", vol(None)),
            ("render/volume/frame_not_minus_1", "volume", vol(key(0))),
            ("render/volume/frame_before_size", "volume", vol(B._render_desc(dict(CAM, width=0), None, 3))),
            ("render/volume/width_0", "volume", vol(free(width=0))),
            ("render/volume/height_too_large", "volume", vol(free(height=32769)))]


def _track_cases(L):
    """i3d_track_frame / _rgbd / i3d_fusion_track and the two i3d_debug_track*_sums"""
    D = lambda **kw: B.track_desc_default(intr=INTR, **kw)
    R = lambda **kw: B.track_rgbd_desc_default(intr=INTR, **kw)

    def shared(kind, stage, fn):
        run = lambda d, w=4, h=4, dep=DEP, pose=True: (lambda hd, o: fn(hd, d, w, h, p(dep), p(o.pose()) if pose else None, o.stats(B.TrackStats)))
        return [(f"track/{kind}/{name}", stage, call) for name, call in [
            ("null_descriptor", run(None)), ("null_depth", run(D(), dep=None)), ("null_pose", run(D(), pose=False)),
            ("levels_0", run(D(levels=0))), ("levels_5", run(D(levels=5))),
            ("iterations_negative", run(D(iterations=[-1]))), ("iterations_101_at_level_1", run(D(levels=2, iterations=[1, 101]))),
            ("width_0", run(D(), w=0)), ("height_too_large", run(D(), h=32769)), ("too_small_for_the_pyramid", run(D(levels=2))),
            ("max_distance_0", run(D(max_distance=0.0))), ("max_distance_nan", run(D(max_distance=NAN))),
            ("focal_0", run(B.track_desc_default(intr=[0.0, 30.0, 1.5, 1.5]))), ("focal_negative", run(B.track_desc_default(intr=[30.0, -1.0, 1.5, 1.5]))),
            ("null_depth_before_levels", run(D(levels=0), dep=None)), ("size_before_max_distance", run(D(max_distance=0.0), w=-1))]]

    def rgbd(d, lum=LUM, dep=DEP, pose=True, w=4):
        return lambda h, o: L.i3d_track_frame_rgbd(h, d, w, 4, p(dep), p(lum), p(o.pose()) if pose else None, o.stats(B.TrackRgbdStats))

    def sums(d, level=0, ref=True, dep=DEP):
        return lambda h, o: L.i3d_debug_track_sums(h, d, 4, 4, p(dep), level, p(o.pose()) if ref else None, p(o.pose()), p(o.arr(29, np.float64)), o.i64())

    def rsums(d, level=0, lum=LUM):
        return lambda h, o: L.i3d_debug_track_rgbd_sums(h, d, 4, 4, p(DEP), p(lum), level, p(o.pose()), p(o.pose()), p(o.arr(31, np.float64)), o.i64(), o.i64())
    own = lambda hd, d, w, h, de, po, st: L.i3d_track_frame(hd, d, w, h, de, po, st)
    fus = lambda hd, d, w, h, de, po, st: L.i3d_fusion_track(hd, d, w, h, de, po, st)
    one = lambda fn, d: (lambda hd, o: fn(hd, d, 4, 4, p(DEP), p(o.pose()), o.stats(B.TrackStats)))
    return shared("context", "grid", own) + shared("volume", "volume", fus) + [
        ("track/context/no_grid", "empty", one(own, D())),
        ("track/context/no_grid_before_focal", "empty", one(own, B.track_desc_default(intr=[0.0, 0.0, 1.5, 1.5]))),
        ("track/context/context_camera_without_a_camera", "grid", one(own, B.track_desc_default())),
        ("track/context/max_distance_before_the_camera", "grid", one(own, B.track_desc_default(max_distance=-1.0))),
        ("track/volume/context_camera", "volume", one(fus, B.track_desc_default())),
        ("track/volume/null_pose_before_context_camera", "volume", lambda hd, o: L.i3d_fusion_track(hd, B.track_desc_default(), 4, 4, p(DEP), None, o.stats(B.TrackStats))),
        ("track_rgbd/null_descriptor", "grid", rgbd(None)), ("track_rgbd/null_pose", "grid", rgbd(R(), pose=False)),
        ("track_rgbd/null_depth", "grid", rgbd(R(), dep=None)), ("track_rgbd/null_luminance", "grid", rgbd(R(), lum=None)),
        ("track_rgbd/weight_negative", "grid", rgbd(R(geometric_weight=-1.0))), ("track_rgbd/weight_nan", "grid", rgbd(R(photo_weight=NAN))),
        ("track_rgbd/weight_inf", "grid", rgbd(R(geometric_weight=INF))), ("track_rgbd/both_weights_0", "grid", rgbd(R(geometric_weight=0.0, photo_weight=0.0))),
        ("track_rgbd/weights_before_levels", "grid", rgbd(R(photo_weight=-1.0, levels=0))), ("track_rgbd/levels_before_size", "grid", rgbd(R(levels=5), w=0)),
        ("track_rgbd/photo_weight_without_sh", "grid", rgbd(R())), ("track_rgbd/no_grid", "empty", rgbd(R())),
        ("track_rgbd/context_camera_without_a_camera", "grid", rgbd(B.track_rgbd_desc_default())),
        ("track_rgbd/sh_before_focal", "keyed", rgbd(B.track_rgbd_desc_default(intr=[0.0, 30.0, 1.5, 1.5]))),
        ("debug_track_sums/null_pose", "grid", sums(D(), ref=False)), ("debug_track_sums/level_out_of_range", "grid", sums(D(), level=1)),
        ("debug_track_sums/level_negative", "grid", sums(D(), level=-1)), ("debug_track_sums/null_depth", "grid", sums(D(), dep=None)),
        ("debug_track_sums/no_grid", "empty", sums(D())), ("debug_track_sums/null_descriptor", "grid", sums(None)),
        ("debug_track_rgbd_sums/null_descriptor", "grid", rsums(None)), ("debug_track_rgbd_sums/level_out_of_range", "grid", rsums(R(), level=1)),
        ("debug_track_rgbd_sums/both_weights_0", "grid", rsums(R(geometric_weight=0.0, photo_weight=0.0))),
        ("debug_track_rgbd_sums/null_luminance", "grid", rsums(R(), lum=None)), ("debug_track_rgbd_sums/photo_weight_without_sh", "keyed", rsums(R()))]


def _query_cases(L):
    """i3d_query_points / i3d_fusion_query_points"""
    D = B.query_desc_default

    def shared(kind, stage, albedo):
        def run(d, n=1, pts=PTS, foot=False):
            def call(h, o):
                out = [p(o.arr(1, np.float64)), p(o.arr((1, 3)))] + ([p(o.arr(1))] if albedo else []) + [p(o.arr((1, 3), np.float64)) if foot else None, None,
                                                                                                       p(o.arr(1, np.uint8))]
                return getattr(L, "i3d_query_points" if albedo else "i3d_fusion_query_points")(h, d, n, p(pts), *out, o.stats(B.QueryStats))
            return call
        return [(f"query/{kind}/{name}", stage, call) for name, call in [
            ("null_descriptor", run(None)), ("n_negative", run(D(), n=-1)), ("n_too_large", run(D(), n=(1 << 27) + 1)), ("null_points", run(D(), pts=None)),
            ("max_steps_negative", run(D(max_steps=-1))), ("max_steps_65", run(D(max_steps=65))),
            ("tolerance_0", run(D(tolerance_voxels=0.0))), ("tolerance_nan", run(D(tolerance_voxels=NAN))), ("tolerance_inf", run(D(tolerance_voxels=INF))),
            ("foot_without_project", run(D(project=0), foot=True)),
            ("null_points_before_max_steps", run(D(max_steps=-1), pts=None)), ("tolerance_before_foot", run(D(project=0, tolerance_voxels=-1.0), foot=True))]], run
    own, run = shared("context", "grid", True)
    vol, _ = shared("volume", "volume", False)
    return own + vol + [("query/context/no_grid", "empty", run(D())), ("query/context/foot_before_no_grid", "empty", run(D(project=0), foot=True))]


def _register_cases(L):
    """i3d_register_points / i3d_fusion_register_points / i3d_debug_register_sums"""
    D = B.register_desc_default

    def shared(kind, stage, fn):
        run = lambda d, n=1, pts=PTS, pose=None, null_pose=False: (lambda h, o: fn(h, d, n, p(pts), None if null_pose else p(o.pose(pose)), o.stats(B.RegisterStats)))
        return [(f"register/{kind}/{name}", stage, call) for name, call in [
            ("null_descriptor", run(None)), ("null_pose", run(D(), null_pose=True)), ("n_negative", run(D(), n=-1)), ("n_too_large", run(D(), n=(1 << 27) + 1)),
            ("null_points", run(D(), pts=None)), ("iterations_negative", run(D(iterations=-1))), ("iterations_201", run(D(iterations=201))),
            ("max_distance_0", run(D(max_distance=0.0))), ("max_distance_nan", run(D(max_distance=NAN))), ("max_distance_inf", run(D(max_distance=INF))),
            ("pose_nan", run(D(), pose=NAN_POSE)), ("pose_inf", run(D(), pose=INF_POSE)),
            ("null_pose_before_n", run(D(), n=-1, null_pose=True)), ("iterations_before_pose", run(D(iterations=-1), pose=NAN_POSE))]], run
    own, run = shared("context", "grid", lambda *a: L.i3d_register_points(*a))
    vol, _ = shared("volume", "volume", lambda *a: L.i3d_fusion_register_points(*a))

    def sums(d, pivot=PIVOT, pose=None, pts=PTS):
        return lambda h, o: L.i3d_debug_register_sums(h, d, 1, p(pts), p(o.pose(pose)), p(pivot), p(o.arr(29, np.float64)), o.i64())
    return own + vol + [
        ("register/context/no_grid", "empty", run(D())), ("register/context/pose_before_no_grid", "empty", run(D(), pose=NAN_POSE)),
        ("debug_register_sums/null_pivot", "grid", sums(D(), pivot=None)), ("debug_register_sums/null_descriptor", "grid", sums(None)),
        ("debug_register_sums/null_points", "grid", sums(D(), pts=None)), ("debug_register_sums/pose_nan", "grid", sums(D(), pose=NAN_POSE)),
        ("debug_register_sums/no_grid", "empty", sums(D()))]


def _track_sdf_cases(L):
    """i3d_track_frame_sdf / _rgbd / i3d_fusion_track_sdf / _rgbd and their i3d_debug_*_sums"""
    D = lambda **kw: B.track_sdf_desc_default(intr=INTR, **kw)
    R = lambda **kw: B.track_sdf_rgbd_desc_default(intr=INTR, **kw)

    def shared(kind, stage, fn):
        run = lambda d, w=4, h=4, dep=DEP, pose=None, null_pose=False: (
            lambda hd, o: fn(hd, d, w, h, p(dep), None if null_pose else p(o.pose(pose)), o.stats(B.TrackSdfStats)))
        return [(f"track_sdf/{kind}/{name}", stage, call) for name, call in [
            ("null_descriptor", run(None)), ("null_depth", run(D(), dep=None)), ("null_pose", run(D(), null_pose=True)),
            ("width_0", run(D(), w=0)), ("height_negative", run(D(), h=-1)), ("width_too_large", run(D(), w=32769)),
            ("stride_0", run(D(stride=0))), ("stride_17", run(D(stride=17))), ("iterations_negative", run(D(iterations=-1))), ("iterations_201", run(D(iterations=201))),
            ("max_distance_0", run(D(max_distance=0.0))), ("max_distance_nan", run(D(max_distance=NAN))), ("max_distance_inf", run(D(max_distance=INF))),
            ("huber_delta_nan", run(D(huber_delta=NAN))), ("huber_delta_inf", run(D(huber_delta=INF))),
            ("pose_nan", run(D(), pose=NAN_POSE)), ("pose_inf", run(D(), pose=INF_POSE)),
            ("focal_0", run(B.track_sdf_desc_default(intr=[0.0, 30.0, 1.5, 1.5]))), ("focal_negative", run(B.track_sdf_desc_default(intr=[30.0, -1.0, 1.5, 1.5]))),
            ("null_depth_before_stride", run(D(stride=0), dep=None)), ("stride_before_pose", run(D(stride=0), pose=NAN_POSE)),
            ("pose_before_focal", run(B.track_sdf_desc_default(intr=[0.0, 0.0, 1.5, 1.5]), pose=INF_POSE))]], run

    def shared_rgbd(kind, stage, fn):
        run = lambda d, w=4, dep=DEP, lum=LUM, pose=None: (lambda hd, o: fn(hd, d, w, 4, p(dep), p(lum), p(o.pose(pose)), o.stats(B.TrackSdfRgbdStats)))
        return [(f"track_sdf_rgbd/{kind}/{name}", stage, call) for name, call in [
            ("null_descriptor", run(None)), ("null_depth", run(R(), dep=None)), ("null_luminance", run(R(), lum=None)), ("stride_0", run(R(stride=0))),
            ("weight_negative", run(R(photo_weight=-1.0))), ("weight_nan", run(R(geometric_weight=NAN))), ("weight_inf", run(R(photo_weight=INF))),
            ("both_weights_0", run(R(geometric_weight=0.0, photo_weight=0.0))), ("max_photo_residual_nan", run(R(max_photo_residual=NAN))),
            ("max_photo_residual_inf", run(R(max_photo_residual=INF))), ("pose_nan", run(R(), pose=NAN_POSE)),
            ("focal_0", run(B.track_sdf_rgbd_desc_default(intr=[0.0, 30.0, 1.5, 1.5]))),
            ("null_luminance_before_size", run(R(), w=0, lum=None)), ("huber_before_weights", run(R(huber_delta=NAN, photo_weight=-1.0))),
            ("weights_before_pose", run(R(geometric_weight=-1.0), pose=NAN_POSE))]], run
    own, run = shared("context", "grid", lambda *a: L.i3d_track_frame_sdf(*a))
    vol, vrun = shared("volume", "volume", lambda *a: L.i3d_fusion_track_sdf(*a))
    own_r, rrun = shared_rgbd("context", "grid", lambda *a: L.i3d_track_frame_sdf_rgbd(*a))
    vol_r, vrrun = shared_rgbd("volume", "volume", lambda *a: L.i3d_fusion_track_sdf_rgbd(*a))
    CC = lambda **kw: B.track_sdf_desc_default(use_context_camera=1, **kw)
    RCC = lambda **kw: B.track_sdf_rgbd_desc_default(use_context_camera=1, **kw)

    def sums(d, pivot=PIVOT, pose=None):
        return lambda h, o: L.i3d_debug_track_sdf_sums(h, d, 4, 4, p(DEP), p(o.pose(pose)), p(pivot), p(o.arr(29, np.float64)), o.i64(), o.i64())

    def rsums(fn, d, pivot=PIVOT, lum=LUM):
        return lambda h, o: fn(h, d, 4, 4, p(DEP), p(lum), p(o.pose()), p(pivot), p(o.arr(31, np.float64)), o.i64(), o.i64())
    own_s = lambda *a: L.i3d_debug_track_sdf_rgbd_sums(*a)
    vol_s = lambda *a: L.i3d_fusion_debug_track_sdf_rgbd_sums(*a)
    return own + vol + own_r + vol_r + [
        ("track_sdf/context/no_grid", "empty", run(D())), ("track_sdf/context/pose_before_no_grid", "empty", run(D(), pose=NAN_POSE)),
        ("track_sdf/context/no_grid_before_focal", "empty", run(B.track_sdf_desc_default(intr=[0.0, 0.0, 1.5, 1.5]))),
        ("track_sdf/context/context_camera_without_a_camera", "grid", run(CC())),
        ("track_sdf/volume/context_camera", "volume", vrun(CC())), ("track_sdf/volume/context_camera_before_null_depth", "volume", vrun(CC(), dep=None)),
        ("track_sdf_rgbd/context/no_grid", "empty", rrun(R())), ("track_sdf_rgbd/context/context_camera_without_a_camera", "grid", rrun(RCC())),
        ("track_sdf_rgbd/context/photo_weight_without_sh", "grid", rrun(R())),
        ("track_sdf_rgbd/context/focal_before_sh", "grid", rrun(B.track_sdf_rgbd_desc_default(intr=[30.0, 0.0, 1.5, 1.5]))),
        ("track_sdf_rgbd/context/context_camera_without_sh", "keyed", rrun(RCC())),
        ("track_sdf_rgbd/volume/context_camera", "volume", vrrun(RCC())), ("track_sdf_rgbd/volume/context_camera_before_weights", "volume", vrrun(RCC(photo_weight=-1.0))),
        ("debug_track_sdf_sums/null_pivot", "grid", sums(D(), pivot=None)), ("debug_track_sdf_sums/null_descriptor", "grid", sums(None)),
        ("debug_track_sdf_sums/stride_0", "grid", sums(D(stride=0))), ("debug_track_sdf_sums/pose_nan", "grid", sums(D(), pose=NAN_POSE)),
        ("debug_track_sdf_sums/no_grid", "empty", sums(D())),
        ("debug_track_sdf_rgbd_sums/null_descriptor", "grid", rsums(own_s, None)), ("debug_track_sdf_rgbd_sums/null_pivot", "grid", rsums(own_s, R(), pivot=None)),
        ("debug_track_sdf_rgbd_sums/null_luminance", "grid", rsums(own_s, R(), lum=None)),
        ("debug_track_sdf_rgbd_sums/both_weights_0", "grid", rsums(own_s, R(geometric_weight=0.0, photo_weight=0.0))),
        ("debug_track_sdf_rgbd_sums/photo_weight_without_sh", "grid", rsums(own_s, R())),
        ("fusion_debug_track_sdf_rgbd_sums/null_descriptor", "volume", rsums(vol_s, None)),
        ("fusion_debug_track_sdf_rgbd_sums/context_camera", "volume", rsums(vol_s, RCC())),
        ("fusion_debug_track_sdf_rgbd_sums/weight_nan", "volume", rsums(vol_s, R(photo_weight=NAN))),
        ("fusion_debug_track_sdf_rgbd_sums/max_photo_residual_nan", "volume", rsums(vol_s, R(max_photo_residual=NAN)))]


def _batch_cases(L):
    """i3d_track_frames_sdf(_rgbd) / i3d_track_keyframes_sdf(_rgbd)"""
    D = lambda **kw: B.track_sdf_desc_default(intr=INTR, **kw)
    R = lambda **kw: B.track_sdf_rgbd_desc_default(intr=INTR, **kw)
    CC = lambda **kw: B.track_sdf_desc_default(use_context_camera=1, **kw)
    RCC = lambda **kw: B.track_sdf_rgbd_desc_default(use_context_camera=1, **kw)
    nan1 = np.zeros((2, 6)); nan1[1, 4] = NAN
    idx = lambda *a: np.array(a, np.int32)

    def frames(d, n=2, w=4, h=4, dep=DEP2, poses=None, null_poses=False):
        return lambda hd, o: L.i3d_track_frames_sdf(hd, d, n, w, h, p(dep), None if null_poses else p(o.pose(poses, 2)), o.stats(B.TrackSdfStats, 2))

    def frames_r(d, w=4, dep=DEP2, lum=LUM2, poses=None):
        return lambda hd, o: L.i3d_track_frames_sdf_rgbd(hd, d, 2, w, 4, p(dep), p(lum), p(o.pose(poses, 2)), o.stats(B.TrackSdfRgbdStats, 2))

    def keys(d, level=0, n=2, fr=idx(0, 1), poses=None, null_poses=False):
        return lambda hd, o: L.i3d_track_keyframes_sdf(hd, d, level, n, p(fr), None if null_poses else p(o.pose(poses, 2)), o.stats(B.TrackSdfStats, 2))

    def keys_r(d, level=0, fr=idx(0, 1), poses=None):
        return lambda hd, o: L.i3d_track_keyframes_sdf_rgbd(hd, d, level, 2, p(fr), p(o.pose(poses, 2)), o.stats(B.TrackSdfRgbdStats, 2))
    return [(f"track_frames_sdf/{name}", stage, call) for name, stage, call in [
        ("null_descriptor", "grid", frames(None)), ("num_negative", "grid", frames(D(), n=-1)), ("null_depth", "grid", frames(D(), dep=None)),
        ("null_poses", "grid", frames(D(), null_poses=True)), ("width_0", "grid", frames(D(), w=0)), ("height_too_large", "grid", frames(D(), h=32769)),
        ("stride_17", "grid", frames(D(stride=17))), ("iterations_201", "grid", frames(D(iterations=201))), ("max_distance_0", "grid", frames(D(max_distance=0.0))),
        ("huber_delta_nan", "grid", frames(D(huber_delta=NAN))), ("pose_of_frame_1_nan", "grid", frames(D(), poses=nan1)),
        ("focal_0", "grid", frames(B.track_sdf_desc_default(intr=[0.0, 30.0, 1.5, 1.5]))), ("no_grid", "empty", frames(D())),
        ("context_camera_without_a_camera", "grid", frames(CC())),
        ("null_depth_before_size", "grid", frames(D(), w=0, dep=None)), ("pose_before_no_grid", "empty", frames(D(), poses=nan1)),
        ("no_grid_before_focal", "empty", frames(B.track_sdf_desc_default(intr=[0.0, 0.0, 1.5, 1.5])))]] + [
        (f"track_frames_sdf_rgbd/{name}", stage, call) for name, stage, call in [
        ("null_descriptor", "grid", frames_r(None)), ("null_luminance", "grid", frames_r(R(), lum=None)), ("stride_0", "grid", frames_r(R(stride=0))),
        ("weight_negative", "grid", frames_r(R(geometric_weight=-1.0))), ("weight_nan", "grid", frames_r(R(photo_weight=NAN))),
        ("both_weights_0", "grid", frames_r(R(geometric_weight=0.0, photo_weight=0.0))), ("max_photo_residual_nan", "grid", frames_r(R(max_photo_residual=NAN))),
        ("photo_weight_without_sh", "grid", frames_r(R())), ("no_grid", "empty", frames_r(R())),
        ("focal_before_weights", "grid", frames_r(B.track_sdf_rgbd_desc_default(intr=[0.0, 30.0, 1.5, 1.5], photo_weight=-1.0))),
        ("pose_before_weights", "grid", frames_r(R(photo_weight=-1.0), poses=nan1))]] + [
        (f"track_keyframes_sdf/{name}", stage, call) for name, stage, call in [
        ("null_descriptor", "keyed", keys(None)), ("num_negative", "keyed", keys(CC(), n=-1)), ("null_poses", "keyed", keys(CC(), null_poses=True)),
        ("own_camera", "keyed", keys(D())), ("no_grid", "empty", keys(CC())), ("no_keyframes", "grid", keys(CC())), ("no_camera", "framed", keys(CC())),
        ("level_negative", "keyed", keys(CC(), level=-1)), ("level_1", "keyed", keys(CC(), level=1)),
        ("index_3", "keyed", keys(CC(), fr=idx(0, 3))), ("index_negative", "keyed", keys(CC(), fr=idx(-1, 0))),
        ("num_without_indices", "keyed", keys(CC(), n=1, fr=None)), ("stride_17", "keyed", keys(CC(stride=17))),
        ("max_distance_negative", "keyed", keys(CC(max_distance=-1.0))), ("pose_of_frame_1_nan", "keyed", keys(CC(), poses=nan1)),
        ("own_camera_before_no_grid", "empty", keys(D())), ("level_before_index", "keyed", keys(CC(), level=2, fr=idx(0, 7))),
        ("index_before_stride", "keyed", keys(CC(stride=0), fr=idx(5, 0)))]] + [
        (f"track_keyframes_sdf_rgbd/{name}", stage, call) for name, stage, call in [
        ("null_descriptor", "keyed", keys_r(None)), ("weight_negative", "keyed", keys_r(RCC(photo_weight=-1.0))),
        ("both_weights_0", "keyed", keys_r(RCC(geometric_weight=0.0, photo_weight=0.0))), ("max_photo_residual_inf", "keyed", keys_r(RCC(max_photo_residual=INF))),
        ("photo_weight_without_sh", "keyed", keys_r(RCC())), ("no_camera", "framed", keys_r(RCC())), ("level_1", "keyed", keys_r(RCC(), level=1)),
        ("pose_before_weights", "keyed", keys_r(RCC(photo_weight=-1.0), poses=nan1))]]


def table(L):
    """every case: (name, stage of the handle it runs on, call(handle, outs) -> return code)"""
    cases = _render_cases(L) + _track_cases(L) + _query_cases(L) + _register_cases(L) + _track_sdf_cases(L) + _batch_cases(L)
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cases


def run_table():
    """the table on its handles -> [{name, code, error, untouched}], in the table's order within each stage"""
    L = B.load()
    cases = table(L)
    out = {}

    def stage(name, handle, last_error):
        for case, _, call in (c for c in cases if c[1] == name):
            o = Outs()
            rc = call(handle.h, o)
            out[case] = dict(name=case, code=int(rc), error=getattr(L, last_error)(handle.h).decode(), untouched=bool(o.untouched()))

    with B.Context(0) as empty:
        stage("empty", empty, "i3d_last_error")
    g = RC.grid("plain")
    with B.Context(0) as ctx:
        ctx.set_grid(RC.VS, g["keys"], g["sdf"], g["sdf_refined"], g["albedo"], g["weight"], g["color"])
        stage("grid", ctx, "i3d_last_error")
        ctx.set_frames([dict(lum=[np.full((4, 4), 0.5, np.float32)], depth=[np.ones((4, 4), np.float32)]) for _ in range(2)], 1)
        stage("framed", ctx, "i3d_last_error")
        ctx.set_camera(INTR, np.zeros(5), np.zeros((2, 6)))
        stage("keyed", ctx, "i3d_last_error")
    scene = FC.fusion_scene()
    pose = FC.orbit_pose(scene, 0.0)
    depth = track_twin.raycast_scene(scene, track_twin.level_camera(FC.INTR, np.zeros(5), FC.W, FC.H, 0), track_twin.ref_from_pose(pose))[0]
    f = FC.fused([(depth, pose)])
    try:
        stage("volume", f, "i3d_fusion_last_error")
    finally:
        f.close()
    return [out[c[0]] for c in cases]


def test_fault_table_equals_the_recorded_one():
    compare_with_golden(GOLDEN, run_table())


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit("usage: test_gpu_model_errors.py --record [path]   (writes the fault table of the loaded library)")
    sys.exit(record_golden(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, run_table(), B.LIB_PATH))
