"""The scene, the frames, the runs and the recorded figures of the tests of i3d_fusion_track_sdf_rgbd: test_fusion_track_sdf_rgbd_cpu.py
asserts their input conditions on the twin, test_gpu_fusion_track_sdf_rgbd.py compares the device on them.

The scene is a smooth sphere of radius 14 voxels at 4 mm (no bumps: its depth is blind to a rotation about its centre) with the textured albedo (albedo_freq 60,
amplitude 0.3).  Four frames rendered by synthetic.render_frame at 0 / 8 / 16 / 24 degrees of test_gpu_query._pose's arc are fused by the oracle's Fusion; the
held-out 12 degree frame is the one tracked, from three starts orbited 2 degrees about the sphere's centre and moved 1 voxel (track_rgbd_twin.orbit, seed 17).
Two image sizes: 96 x 72 and 64 x 48.

A frame is CHECKED as in track_sdf_rgbd_cases: every sample that at any sums pass of any twin run listed for it lies within FACE_MARGIN voxel of a cell face,
GATE_MARGIN vs of the gate or of huber_delta, or PHOTO_GATE_MARGIN of the photo gate has its depth set to 0, until none is left.
"""
import functools
import math

import numpy as np

import fusion_track_sdf_rgbd_twin as FT
import track_rgbd_twin
import track_sdf_rgbd_cases as PC
import track_sdf_twin as ST
from intrinsic3d_amd import synthetic

VS = 0.004
RADIUS_VOX = 14
SIZES = ((96, 72), (64, 48))
FUSED_DEG = (0.0, 8.0, 16.0, 24.0)
TRACKED_DEG = 12.0
BUDGET = 60
HUBER = 0.5 * VS
PHOTO_GATE = 0.05             # luminance units: at the start poses it cuts a part of the photometric samples, not all (asserted by the CPU test)
MAX_REMOVED = PC.MAX_REMOVED
FACE_MARGIN, GATE_MARGIN, PHOTO_GATE_MARGIN = PC.FACE_MARGIN, PC.GATE_MARGIN, PC.PHOTO_GATE_MARGIN
DIST = np.zeros(5)

# Recorded by test_fusion_track_sdf_rgbd_cpu.py: the twin's rotation error against the truth, degrees, of the colour run at 64 x 48 from the
# three starts (one pose from all three), seven digits.  DEVICE_TWIN_BAR: the device's error may be that times 1.001.  The issue allowed 1.5 for the summation
# order through a 6-step loop near a flat minimum; measured on the MI355X the device / twin ratio is 1.000000 from all three starts (the poses differ by 1e-15
# rad, section 22.3), so the bar is the rounding of the recorded figure (4e-7 relative) with room, not the issue's
TWIN_ERR_DEG_64 = (0.2668013, 0.2668013, 0.2668013)
DEVICE_TWIN_BAR = 1.001

DEPTH_ONLY = dict(photo_weight=0.0, iterations=BUDGET)
COLOUR = dict(iterations=BUDGET)
ONE_PASS = [dict(stride=2, iterations=0), dict(stride=3, iterations=0), dict(huber_delta=HUBER, iterations=0), dict(max_photo_residual=PHOTO_GATE, iterations=0),
            dict(geometric_weight=0.0, iterations=0), dict(stride=2, huber_delta=HUBER, max_photo_residual=PHOTO_GATE, iterations=0)]
# (width, height, start) -> the runs whose passes the check covers and the device test repeats; "px1", "row65", "nan": the frames of the sums test alone
FRAMES = {(w, h, k): [DEPTH_ONLY, COLOUR] + (ONE_PASS if (w, h, k) == (64, 48, 0) else []) for w, h in SIZES for k in range(3)}
FRAMES[("px1", 0, 0)] = [dict(iterations=0)]
FRAMES[("row65", 0, 0)] = [dict(iterations=0), dict(stride=2, iterations=0)]
FRAMES[("nan", 0, 0)] = [dict(iterations=0), dict(huber_delta=HUBER, iterations=0)]
FULL_FRAMES = [k for k in FRAMES if isinstance(k[0], int)]


def scene():
    return synthetic.Scene(np.full(3, (RADIUS_VOX + 10) * VS), RADIUS_VOX * VS, 0.0, 40.0, albedo_freq=60.0, albedo_amp=0.3)


def intrinsics(w, h):
    fx = 525.0 * w / 640.0
    return np.array([fx, fx, (w - 1) * 0.5, (h - 1) * 0.5])


def arc_pose(theta_deg, w, h, elev_deg=20.0):
    """test_gpu_query._pose: the sphere fills 0.35 of the image height on either side of the centre"""
    sc = scene()
    th, el = math.radians(theta_deg), math.radians(elev_deg)
    d = sc.R * intrinsics(w, h)[0] / (0.35 * h)
    return synthetic.look_at_pose(sc.c + d * np.array([math.sin(th) * math.cos(el), math.sin(el), math.cos(th) * math.cos(el)]), sc.c)


def c2w(pose):
    R = synthetic.aa_to_rotmat(np.asarray(pose[:3], np.float64))
    M = np.eye(4); M[:3, :3] = R.T; M[:3, 3] = -R.T @ np.asarray(pose[3:], np.float64)
    return M.astype(np.float32)


@functools.lru_cache(maxsize=None)
def fused_frames(w, h):
    """[(depth fp32, bgr uint8 grey, world -> camera pose)] of the four fused frames"""
    out = []
    for th in FUSED_DEG:
        p = arc_pose(th, w, h)
        _, depth, bgr = synthetic.render_frame(scene(), p, intrinsics(w, h), w, h)
        out.append((depth, bgr, p))
    return out


def channels(bgr):
    """three channels that differ, from a grey image: B = g, G = 255 - g, R = g / 2"""
    g = bgr[..., 0]
    return np.stack([g, 255 - g, g // 2], -1).astype(np.uint8)


def fuse(fusion, w, h, frames=None, colour=None):
    """integrates the frames (default: the four fused ones) into a Fusion of the library or of the oracle"""
    intr = intrinsics(w, h).astype(np.float32)
    for depth, bgr, p in fused_frames(w, h) if frames is None else frames:
        fusion.integrate(depth, intr, bgr if colour is None else colour(bgr), intr, c2w(p), 2)
    return fusion


@functools.lru_cache(maxsize=None)
def volume(w, h, differ=False):
    """the oracle's volume of the four frames as the table holds it after finish(0): dict(keys, sdf, weight, color) of the voxels with weight != 0"""
    from oracle import oracle_py as O
    O.build()
    f = fuse(O.Fusion(VS, 0.1, 10.0), w, h, colour=channels if differ else None)
    f.finish(0)
    return f.export()


@functools.lru_cache(maxsize=None)
def raw_volume(w, h, differ=False):
    """the same volume before finish: every allocated voxel, those with weight 0 included (stored, without a luminance)"""
    from oracle import oracle_py as O
    O.build()
    return fuse(O.Fusion(VS, 0.1, 10.0), w, h, colour=channels if differ else None).export()


@functools.lru_cache(maxsize=None)
def twin(w, h):
    ex = volume(w, h)
    return FT.grid_of(ex, VS), FT.voxel_luminance(ex)


@functools.lru_cache(maxsize=None)
def tracked_frame(w, h):
    """(cam, depth, lum, truth) of the held-out frame; lum is what app_fusion forms from the colour image"""
    truth = arc_pose(TRACKED_DEG, w, h)
    intr = intrinsics(w, h)
    _, depth, bgr = synthetic.render_frame(scene(), truth, intr, w, h)
    i32 = intr.astype(np.float32)
    return dict(width=w, height=h, intr=intr, dist=DIST, pose=truth), depth, FT.frame_luminance(bgr, i32, i32, w, h), truth


def starts(w, h):
    rng = np.random.default_rng(17)
    truth = arc_pose(TRACKED_DEG, w, h)
    return [track_rgbd_twin.orbit(truth, scene().c, rng, 2.0, 1.0 * VS) for _ in range(3)]


def raw_frame(key):
    """(volume size, cam, depth, lum, start) of a frame of FRAMES before the check"""
    if isinstance(key[0], int):
        w, h, k = key
        cam, depth, lum, _ = tracked_frame(w, h)
        return (w, h), cam, depth.copy(), lum, starts(w, h)[k]
    w, h = 64, 48
    cam, depth, lum, truth = tracked_frame(w, h)
    start = starts(w, h)[0]
    if key[0] == "nan":                                      # a block and a scatter of pixels without a luminance: no photometric sample there
        lum = lum.copy(); lum[20:28, 24:40] = np.nan; lum.reshape(-1)[::7] = np.nan
        return (w, h), cam, depth.copy(), lum, start
    fx = intrinsics(w, h)[0]
    # the middle row of the 64 x 48 view as an image of its own, and one pixel of it (tail lanes: 65 and 1 samples in a workgroup of 256)
    intr = np.array([fx, fx, 32.0, 0.0]) if key[0] == "row65" else np.array([fx, fx, -3.0, 0.0])
    ww = 65 if key[0] == "row65" else 1
    _, depth, bgr = synthetic.render_frame(scene(), truth, intr, ww, 1)
    i32 = intr.astype(np.float32)
    return (w, h), dict(width=ww, height=1, intr=intr, dist=DIST, pose=truth), depth, FT.frame_luminance(bgr, i32, i32, ww, 1), start


@functools.lru_cache(maxsize=None)
def checked_frame(key):
    """(volume size, cam, depth [h, w] fp32 checked, lum [h, w] fp32, start pose (world -> camera), [(desc, twin pose, twin stats with trace)] for the frame's
    runs, share of the usable pixels the check removed)"""
    size, cam, depth, lum, start = raw_frame(key)
    grid, vol = twin(*size)
    usable0 = int((depth > 0).sum())
    for _ in range(50):
        runs, bad = [], np.zeros(depth.size, bool)
        for desc in FRAMES[key]:
            pose, st = FT.track(grid, vol, depth, lum, cam["intr"], cam["dist"], start, desc, trace=True)
            face, gate, photo = PC.run_margins(grid, st, desc)
            bad[st["index"][(face < FACE_MARGIN) | (gate < GATE_MARGIN) | (photo < PHOTO_GATE_MARGIN)]] = True
            runs.append((desc, pose, st))
        if not bad.any():
            return size, cam, depth, lum, start, runs, 1.0 - int((depth > 0).sum()) / max(usable0, 1)
        depth.reshape(-1)[bad] = 0.0
    raise AssertionError("the check did not settle")


def order_bar(key, i):
    """track_sdf_rgbd_cases.order_bar's rule: 100 x the pose difference between the twin with numpy's sums and with sequential sums, floor 1e-12 (rad, voxel)"""
    size, cam, depth, lum, start, runs, _ = checked_frame(key)
    desc, pose, st = runs[i]
    grid, vol = twin(*size)
    seq, st2 = FT.track(grid, vol, depth, lum, cam["intr"], cam["dist"], start, desc, order="sequential")
    assert st2["status"] == st["status"] and st2["iterations"] == st["iterations"], (key, i, st2["status"], st["status"], st2["iterations"], st["iterations"])
    ang, tr = ST.pose_err(seq, pose, VS)
    return max(100.0 * ang, 1e-12), max(100.0 * tr, 1e-12), (ang, tr)


def twin_start_sums(key, i, order="numpy"):
    """the twin's pass at the start pose of run i, about the run's pivot: (sums dict, pivot)"""
    size, cam, depth, lum, start, runs, _ = checked_frame(key)
    desc, _, st = runs[i]
    d = FT.default_desc(**desc)
    R, t = ST.pose_to_cw(start)
    c = st["pivot"]
    return FT.PT.sums(twin(*size)[0], st["vol"], st["points"], st["lum"], R, t - c, c, d["max_distance"], d["huber_delta"], d["geometric_weight"], d["photo_weight"],
                      d["max_photo_residual"], order), c
