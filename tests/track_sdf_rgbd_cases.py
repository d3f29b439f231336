"""The frames, the runs and the recorded bars of the tests of i3d_track_frame_sdf_rgbd (test_track_sdf_rgbd_cpu.py asserts their input conditions and measures the
bars, test_gpu_track_sdf_rgbd.py compares the device on them).

The shell models are register_cases' three bumpy-sphere shells with the constant lighting synthetic.SH_TRUE at every voxel, seen through track_sdf_cases' cameras;
the smooth model is track_cases.smooth_scene (a sphere without bumps, a full band, the scene's albedo) seen at 80 x 60.  A frame is the render twin's fp32
depth and intensity of the model at the view's pose.

A frame is CHECKED as in track_sdf_cases: every sample whose placed point, at any sums pass of any twin run listed for the frame, lies within FACE_MARGIN voxel of
a cell face, or whose |r| lies within GATE_MARGIN * vs of the gate or of huber_delta, or whose |r_p| lies within PHOTO_GATE_MARGIN of the photo gate where the run
sets one, has its depth set to 0, until none is left.  At most MAX_REMOVED of the usable samples may go this way (asserted by the CPU test).
"""
import functools

import numpy as np

import query_cases as Q
import register_cases as RC
import render_twin
import track_cases as TR
import track_sdf_cases as SC
import track_sdf_rgbd_twin as PT
import track_sdf_twin as ST
import track_twin
from intrinsic3d_amd import synthetic

VS = RC.VS
FACE_MARGIN = RC.FACE_MARGIN
GATE_MARGIN = RC.GATE_MARGIN
PHOTO_GATE_MARGIN = 1e-9      # luminance units
MAX_REMOVED = SC.MAX_REMOVED
ROW_CAP_P2 = SC.ROW_CAP_P2
HUBER = SC.HUBER
PHOTO_GATE = 0.004            # luminance units: at the shells' start pose it cuts a part of the photometric samples, not all (asserted where it is used)

# Recorded by test_track_sdf_rgbd_cpu.py.  Twin against the render pose over the shell runs of TRUTH_RUNS: rotation <= 4.38e-4 rad, camera
# centre <= 1.30e-2 voxel; the device's bars are twice that, rounded up.  Above the depth-only bars of section 19.3 (4e-5 rad): the frame's intensity is the
# renderer's (albedo and SH interpolated, the interpolant's normal) and the model's is the per-voxel product, which differ by the curvature of both inside a cell.
TRUTH_BAR_RAD, TRUTH_BAR_VOX = 9e-4, 2.7e-2
# The smooth scene (80 x 60, three starts 2 degrees about the centre and 2.4 to 4.1 voxels off, stop 1e-6, budget 60): the twin ends 3.67e-4 rad / 1.85e-2 voxel
# from the truth from every start; twice that, rounded up.
SMOOTH_BAR_RAD, SMOOTH_BAR_VOX = 8e-4, 3.8e-2

SMOOTH_BUDGET = 60
SMOOTH_W, SMOOTH_H = 80, 60


def sh_of(n):
    return np.tile(synthetic.SH_TRUE, (n, 1))


# ---- the models ------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def smooth():
    return TR.smooth_scene()


def model(name):
    """dict(keys, sdf, sdf_refined, albedo, weight, color, sh) of a model: one of register_cases' grids, or "smooth" """
    if name == "smooth":
        sc = smooth()
        n = sc["keys"].shape[0]
        sdf = sc["sdf"].astype(np.float64)
        return dict(keys=sc["keys"], sdf=sdf, sdf_refined=sdf, albedo=np.asarray(sc["albedo_true"], np.float64), weight=sc["weight"], color=sc["color"], sh=sh_of(n),
                    voxel_size=float(sc["voxel_size"]))
    g = RC.grid(name)
    return dict(g, sh=sh_of(g["keys"].shape[0]), voxel_size=VS)


def twin_grid(name, refined=True, albedo=None):
    m = model(name)
    return render_twin.Grid(m["keys"], m["sdf_refined"] if refined else m["sdf"], m["weight"], m["voxel_size"], albedo=m["albedo"] if albedo is None else albedo,
                            sh=m["sh"])


def camera(name, kind):
    if name != "smooth":
        return SC.camera(RC.grid(name), kind)
    sc = smooth()
    lc = track_twin.level_camera(sc["intr"], np.zeros(5), sc["width"], sc["height"], 1)
    assert (lc["w"], lc["h"]) == (SMOOTH_W, SMOOTH_H)
    return dict(width=lc["w"], height=lc["h"], intr=lc["intr"], dist=lc["dist"], pose=np.asarray(sc["truth"], np.float64))


def start_pose(name, kind, k=0):
    if name != "smooth":
        return SC.start_pose(RC.grid(name), camera(name, kind))
    return np.asarray(TR.smooth_starts(smooth())[k], np.float64)


@functools.lru_cache(maxsize=None)
def rendered(name, kind, refined):
    """the render twin's fp32 depth and intensity planes of the view"""
    cam = camera(name, kind)
    rt = render_twin.render(twin_grid(name, refined), render_twin.camera_from_pose(cam["pose"], cam["intr"], cam["dist"], cam["width"], cam["height"]))
    shape = (cam["height"], cam["width"])
    return np.asarray(rt["depth"], np.float32).reshape(shape), np.asarray(rt["intensity"], np.float32).reshape(shape)


# ---- the frames: (model, camera, refined, start) -> the runs (descriptor fields) whose passes the check covers and the device test repeats ------------------
GATED = dict(max_photo_residual=PHOTO_GATE, iterations=0)
PHOTO_ONLY = dict(geometric_weight=0.0, iterations=0)
SMOOTH_RUNS = [dict(photo_weight=0.0, iterations=SMOOTH_BUDGET), dict(iterations=SMOOTH_BUDGET)]
FRAMES = {
    ("plain", "plain32", True, 0): [dict(stride=1), dict(stride=2), dict(stride=3, iterations=0), dict(huber_delta=HUBER), GATED, PHOTO_ONLY],
    ("shifted", "dist32", True, 0): [dict(stride=1), dict(stride=2), dict(stride=3, iterations=0), dict(huber_delta=HUBER, iterations=0)],
    ("shifted", "plain32", True, 0): [dict(stride=1)],
    ("negative", "plain32", True, 0): [dict(stride=1)],
    ("negative", "plain32", False, 0): [dict(stride=1), GATED],
    ("plain", "plain64", True, 0): [dict(stride=1), dict(huber_delta=HUBER, iterations=0)],
    ("plain", "px1", True, 0): [dict(iterations=0)],
    ("plain", "row65", True, 0): [dict(iterations=0), dict(stride=2, iterations=0)],
    ("smooth", "level1", True, 0): SMOOTH_RUNS,
    ("smooth", "level1", True, 1): SMOOTH_RUNS,
    ("smooth", "level1", True, 2): SMOOTH_RUNS,
}
SHELL_FRAMES = [k for k in FRAMES if k[0] != "smooth"]
SMOOTH_FRAMES = [k for k in FRAMES if k[0] == "smooth"]
# the runs with a budget on the 32 x 24 shells: against the twin and against the render pose
TRUTH_RUNS = [(("plain", "plain32", True, 0), 0), (("plain", "plain32", True, 0), 1), (("shifted", "dist32", True, 0), 0), (("shifted", "dist32", True, 0), 1),
              (("shifted", "plain32", True, 0), 0), (("negative", "plain32", True, 0), 0), (("negative", "plain32", False, 0), 0)]
# The limit cycle of section 21.3: on a thin shell the photometric sample set changes between passes, so the steps need not shrink below the stop rule.  What the
# twin does on each run (status, steps) is in test_track_sdf_rgbd_cpu.py; the device must do the same.


def run_margins(grid_tw, st, desc):
    """per sample over the passes of a traced twin run: track_sdf_cases.run_margins, and the smallest distance of |r_p| to the photo gate"""
    d = PT.default_desc(**desc)
    face, gate = SC.run_margins(grid_tw, st, {k: v for k, v in desc.items() if k in ST.default_desc()})
    photo = np.full(face.shape[0], np.inf)
    if d["max_photo_residual"] > 0.0 and d["photo_weight"] > 0.0:
        for a in st["trace"]:
            photo = np.where(a["rp_mask"], np.minimum(photo, np.abs(np.abs(a["rp"]) - d["max_photo_residual"])), photo)
    return face, gate, photo


@functools.lru_cache(maxsize=None)
def checked_frame(key):
    """(cam, depth [h, w] fp32 checked, lum [h, w] fp32, start pose (world -> camera), [(desc, twin pose, twin stats with trace)] for the frame's runs, share of
    the usable pixels the check removed)"""
    name, kind, refined, k = key
    cam = camera(name, kind)
    tw_grid = twin_grid(name, refined)
    depth, lum = rendered(name, kind, refined)
    depth = depth.copy()
    usable0 = int((depth > 0).sum())
    start = start_pose(name, kind, k)
    for _ in range(50):
        runs, bad = [], np.zeros(depth.size, bool)
        for desc in FRAMES[key]:
            pose, st = PT.track(tw_grid, depth, lum, cam["intr"], cam["dist"], start, desc, trace=True)
            face, gate, photo = run_margins(tw_grid, st, desc)
            bad[st["index"][(face < FACE_MARGIN) | (gate < GATE_MARGIN) | (photo < PHOTO_GATE_MARGIN)]] = True
            runs.append((desc, pose, st))
        if not bad.any():
            return cam, depth, lum, start, runs, 1.0 - int((depth > 0).sum()) / max(usable0, 1)
        depth.reshape(-1)[bad] = 0.0
    raise AssertionError("the check did not settle")


def order_bar(key, i):
    """track_sdf_cases.order_bar's rule: 100 x the pose difference between the twin with numpy's sums and with sequential sums, floor 1e-12 (rad, voxel)"""
    cam, depth, lum, start, runs, _ = checked_frame(key)
    desc, pose, st = runs[i]
    seq, st2 = PT.track(twin_grid(key[0], key[2]), depth, lum, cam["intr"], cam["dist"], start, desc, order="sequential")
    assert st2["status"] == st["status"] and st2["iterations"] == st["iterations"], (key, i, st2["status"], st["status"], st2["iterations"], st["iterations"])
    ang, tr = ST.pose_err(seq, pose, model(key[0])["voxel_size"])
    return max(100.0 * ang, 1e-12), max(100.0 * tr, 1e-12), (ang, tr)


translation_quantum = SC.translation_quantum


def twin_start_sums(key, i, order="numpy"):
    """the twin's pass at the start pose of run i, about the run's pivot: (sums dict, pivot)"""
    cam, depth, lum, start, runs, _ = checked_frame(key)
    desc, _, st = runs[i]
    d = PT.default_desc(**desc)
    R, t = ST.pose_to_cw(start)
    c = st["pivot"]
    return PT.sums(twin_grid(key[0], key[2]), st["vol"], st["points"], st["lum"], R, t - c, c, d["max_distance"], d["huber_delta"], d["geometric_weight"],
                   d["photo_weight"], d["max_photo_residual"], order), c
