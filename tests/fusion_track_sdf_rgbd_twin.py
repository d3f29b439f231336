"""numpy statement of i3d_fusion_track_sdf_rgbd: i3d_track_frame_sdf_rgbd's twin (track_sdf_rgbd_twin.py) with the intensity volume replaced by
the luminance of the fusion volume's fused colour.

Test infrastructure: k_fusion_voxel_luminance and the FusionRenderGrid instantiation of the PHOTO sums (track_sdf_kernels.hip) are compared against this.  The
volume is an export of the fusion volume (keys, sdf, weight, colour as R, G, B): the voxels with weight != 0, which are the only ones a cell or a luminance value
can come from.
"""
from __future__ import annotations

import math

import numpy as np

import render_twin
import track_sdf_rgbd_twin as PT
import track_sdf_twin as ST
import track_twin

MIN_INLIERS = PT.MIN_INLIERS
default_desc = PT.default_desc


def luminance(rgb):
    """section 22.1 item 1 on uint8 [..., 3] R, G, B: k_lum_from_bgr's fp32 operations in its order, widened to fp64"""
    c = np.asarray(rgb, np.uint8).astype(np.float32)
    s = np.float32(1.0 / 255.0)
    r, g, b = c[..., 0] * s, c[..., 1] * s, c[..., 2] * s
    return ((b * np.float32(0.114) + g * np.float32(0.587)) + r * np.float32(0.299)).astype(np.float64)


def voxel_luminance(export):
    """c [n] in the export's order, NaN where the weight is 0"""
    return np.where(np.asarray(export["weight"], np.float32) != 0.0, luminance(export["color"]), np.nan)


def grid_of(export, voxel_size):
    """the export as the twin's grid: the float sdf widened to fp64"""
    return render_twin.Grid(export["keys"], np.asarray(export["sdf"], np.float32).astype(np.float64), export["weight"], voxel_size)


def lookup(grid, vol, keys):
    """vol at voxel keys [m, 3], NaN where the key is not stored: what i3d_fusion_debug_voxel_luminance returns"""
    i = grid.find(np.asarray(keys, np.int64))
    return np.where(i >= 0, vol[np.where(i >= 0, i, 0)], np.nan)


def frame_luminance(bgr, dcam, ccam, w, h):
    """the luminance of a colour image [ch, cw, 3] (B, G, R) at the depth camera's geometry, fp32 [h, w]: the colour pixel of depth pixel (u, v) by k_integrate's
    lookup at any depth (the cameras share a centre), round_trunc(((u - cx_d) / fx_d) fx_c + cx_c) in fp32; NaN outside the colour image.  What app_fusion forms"""
    d = [np.float32(x) for x in dcam]; c = [np.float32(x) for x in ccam]
    ch, cw = bgr.shape[:2]
    u = np.arange(w, dtype=np.float32); v = np.arange(h, dtype=np.float32)
    px = np.trunc(((u - d[2]) / d[0]) * c[0] + c[2] + np.float32(0.5)).astype(np.int64)
    py = np.trunc(((v - d[3]) / d[1]) * c[1] + c[3] + np.float32(0.5)).astype(np.int64)
    ok = ((py >= 0) & (py < ch))[:, None] & ((px >= 0) & (px < cw))[None, :]
    pix = np.asarray(bgr, np.uint8)[np.clip(py, 0, ch - 1)[:, None], np.clip(px, 0, cw - 1)[None, :]]
    return np.where(ok, luminance(pix[..., ::-1]), np.nan).astype(np.float32)


def _rms(sq, n):
    return math.sqrt(sq / n) if n > 0 else 0.0


def track(grid, vol, depth, lum, intr, dist, pose6, desc=None, order="numpy", trace=False):
    """i3d_fusion_track_sdf_rgbd.  grid, vol: grid_of and voxel_luminance of one export.  The loop is track_sdf_rgbd_twin.track's over that volume: the same sums
    and solve, the same stats and trace"""
    d = default_desc() if desc is None else default_desc(**desc)
    wg, wp, gate = d["geometric_weight"], d["photo_weight"], d["max_photo_residual"]
    pose6 = np.asarray(pose6, np.float64)
    pts, usable, idx = ST.samples(depth, intr, dist, d["stride"], d["min_depth"], d["max_depth"])
    lum_s = PT.luminance_samples(lum, idx)
    vol = vol if wp > 0.0 else None
    R, t = ST.pose_to_cw(pose6)
    c = ST.pivot(grid, pts, R, t)
    tp = np.array([t[a] - c[a] for a in range(3)])
    st = dict(iterations=0, status=1, valid_pixels=int(usable.sum()), valid=0, inliers=0, rms_initial=0.0, rms_final=0.0, min_pivot_ratio=0.0, photo_samples=0,
              photo_rms_initial=0.0, photo_rms_final=0.0)
    one = lambda: PT.sums(grid, vol, pts, lum_s, R, tp, c, d["max_distance"], d["huber_delta"], wg, wp, gate, order)  # noqa: E731
    tr, steps = [], []
    n_it, status = 0, 1
    for k in range(d["iterations"]):
        a = one()
        tr.append(a)
        if k == 0:
            st["rms_initial"] = _rms(a["sums"][27], a["sums"][28]); st["photo_rms_initial"] = _rms(a["sums"][29], a["sums"][30])
        s, x, ratio = PT.solve(a["sums"], wg)
        if s == 2:
            status = 2
            break
        st["min_pivot_ratio"] = ratio
        if s == 3:
            status = 3
            break
        R, tp = track_twin.apply_step(R, tp, x)
        n_it += 1
        nw = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]); nu = math.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5])
        steps.append((nw, nu))
        if nw < d["stop_rotation"] and nu < d["stop_translation"]:
            status = 0
            break
    a = one()
    tr.append(a)
    st.update(iterations=n_it, valid=a["valid"], inliers=a["inliers"], rms_final=_rms(a["sums"][27], a["sums"][28]), photo_samples=a["samples"],
              photo_rms_final=_rms(a["sums"][29], a["sums"][30]))
    if d["iterations"] == 0:
        st["rms_initial"] = st["rms_final"]; st["photo_rms_initial"] = st["photo_rms_final"]
        status = 2 if (a["inliers"] if wg > 0.0 else a["samples"]) < MIN_INLIERS else 1
    st["status"] = status
    if trace:
        st["trace"] = tr; st["steps"] = steps; st["pivot"] = c; st["points"] = pts; st["index"] = idx; st["lum"] = lum_s; st["vol"] = vol
    out = track_twin.cw_to_pose(R, np.array([tp[a_] + c[a_] for a_ in range(3)])) if n_it > 0 else pose6.copy()
    return out, st
