"""numpy statement of i3d_track_frame_sdf, vectorised over the samples of the depth image, in fp64.

Test infrastructure: the device kernels (track_sdf_kernels.hip, the step of track_kernels.hip) are compared against this.  The samples are the pixels on the
stride lattice, back-projected along render_twin.rays of the identity pose; a sample that is not usable is a NaN point, which section 18 ignores, so the sample
array has one row per sample whatever the depth holds and the order of the sums depends on the image size and the stride alone.  Residual, Jacobian and loop are
register_twin's (section 18.1) on that array with the camera -> world inverse of the given world -> camera pose; the Huber weight multiplies the 27 entries of the
system.  Only the order of the sums over the samples differs from the kernel (numpy's here, or sequential with order="sequential").
"""
from __future__ import annotations

import math

import numpy as np

import query_twin
import register_twin as RT
import render_twin
import track_twin

MIN_INLIERS = RT.MIN_INLIERS
UPPER = RT.UPPER


def default_desc(**kw):
    """i3d_track_sdf_desc_default (the camera is an argument of its own here)"""
    d = dict(iterations=30, stride=1, max_distance=0.05, huber_delta=0.0, min_depth=0.0, max_depth=0.0, stop_rotation=1e-6, stop_translation=1e-6)
    d.update(kw)
    return d


def rotation(aa):
    """R(omega) as the driver forms it (frame_math.hpp frame_from_pose: the rotation of the three basis vectors by the angle-axis formula, in Python floats so that
    every operation and sin / cos are the host's), row-major [3, 3].  synthetic.aa_to_rotmat gives the same matrix to rounding only, and on a grid far from the
    origin one ulp of R moves -R^T t by an ulp of the translation, which every sample then carries."""
    w = [float(x) for x in aa]
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    R = np.zeros((3, 3))
    for col in range(3):
        p = [0.0, 0.0, 0.0]; p[col] = 1.0
        if th2 > 2.220446049250313e-16:
            th = math.sqrt(th2); ct = math.cos(th); st = math.sin(th); ti = 1.0 * (1.0 / th)
            k = [w[0] * ti, w[1] * ti, w[2] * ti]
            kxp = [k[1] * p[2] - k[2] * p[1], k[2] * p[0] - k[0] * p[2], k[0] * p[1] - k[1] * p[0]]
            tmp = ((k[0] * p[0] + k[1] * p[1]) + k[2] * p[2]) * (1.0 - ct)
            o = [(p[i] * ct + kxp[i] * st) + k[i] * tmp for i in range(3)]
        else:
            wxp = [w[1] * p[2] - w[2] * p[1], w[2] * p[0] - w[0] * p[2], w[0] * p[1] - w[1] * p[0]]
            o = [p[i] + wxp[i] for i in range(3)]
        R[:, col] = o
    return R


def pose_to_cw(pose6):
    """world->camera (angle-axis | t) -> camera->world (Rc, tc), the driver's inversion (track.cpp pose_from_vec6) to the bit"""
    R = rotation(pose6[:3])
    t = [float(x) for x in pose6[3:]]
    tc = np.array([-((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2]) for a in range(3)])
    return R.T.copy(), tc


def sample_index(w, h, stride):
    """flat pixel index of every sample, row-major over the lattice: ws = ceil(w / stride), hs = ceil(h / stride)"""
    ws, hs = -(-w // stride), -(-h // stride)
    vv, uu = np.meshgrid(np.arange(hs) * stride, np.arange(ws) * stride, indexing="ij")
    return (vv * w + uu).ravel()


def samples(depth, intr, dist, stride=1, min_depth=0.0, max_depth=0.0):
    """(points [n, 3] in the camera frame, NaN rows where the sample is not usable; usable [n]; pixel index [n])"""
    z32 = np.asarray(depth, np.float32)
    h, w = z32.shape
    ident = dict(R=np.eye(3), eye=np.zeros(3), intr=np.asarray(intr, np.float64), dist=np.asarray(dist, np.float64), w=w, h=h)
    ray, _ = render_twin.rays(ident)                     # (x, y, 1) of every pixel
    idx = sample_index(w, h, stride)
    z = z32.reshape(-1)[idx]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(z) & (z > 0)
        if min_depth > 0:
            ok &= ~(z < np.float32(min_depth))
        if max_depth > 0:
            ok &= ~(z > np.float32(max_depth))
    zd = np.where(ok, z, 1.0).astype(np.float64)
    r = ray[idx]
    p = np.stack([r[:, 0] * zd, r[:, 1] * zd, zd], -1)
    p[~ok] = np.nan
    return p, ok, idx


def pivot(grid, pts, R0, t0):
    """c = R0 mean(p) + t0 over the usable samples that count (register_twin.counted)"""
    ok = RT.counted(grid, pts, R0, t0)
    m = pts[ok].sum(0) / float(ok.sum()) if ok.any() else np.zeros(3)
    return np.array([((R0[a, 0] * m[0] + R0[a, 1] * m[1]) + R0[a, 2] * m[2]) + t0[a] for a in range(3)])


def sums(grid, pts, R, tp, c, max_distance, huber_delta=0.0, order="numpy"):
    """one pass of k_track_sdf at the camera -> world pose (R, t' = t - c) about the pivot c over the sample array: register_twin.sums, with the 27 entries of
    the system multiplied by the Huber weight when huber_delta > 0 (no multiplication otherwise).  Adds "usable" and "weight" [n] (1 where off or not an inlier)."""
    usable = int(np.isfinite(pts).all(1).sum())
    if not huber_delta > 0.0:
        a = RT.sums(grid, pts, R, tp, c, max_distance, order)
        a["usable"] = usable; a["weight"] = np.ones(pts.shape[0])
        return a
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    vs = grid.vs
    with np.errstate(invalid="ignore", over="ignore"):
        xp = RT._place(R, tp, p)
        x = np.stack([xp[:, a] + c[a] for a in range(3)], -1)
    ok, _, v, fr, q = query_twin._locate(grid, x)
    r = np.where(ok, query_twin._tri(query_twin._weights(fr), v), 0.0)
    gr, _ = query_twin._gradient(v, fr)
    inl = ok & (np.abs(r) <= max_distance)
    xi, ri = xp[inl], r[inl]
    ar = np.abs(ri)
    with np.errstate(divide="ignore", invalid="ignore"):
        om = np.where(ar <= huber_delta, 1.0, huber_delta / ar)
    d = [gr[inl][:, a] / vs for a in range(3)]
    J = [xi[:, 1] * d[2] - xi[:, 2] * d[1], xi[:, 2] * d[0] - xi[:, 0] * d[2], xi[:, 0] * d[1] - xi[:, 1] * d[0], d[0], d[1], d[2]]
    terms = [om * (J[a] * J[b]) for a, b in UPPER] + [om * (J[a] * ri) for a in range(6)] + [ri * ri, np.ones_like(ri)]
    T = np.stack(terms, -1) if ri.size else np.zeros((0, 29))
    if order == "sequential":
        tot = np.zeros(29)
        for row in T:
            tot = tot + row
    else:
        tot = np.ascontiguousarray(T.T).sum(1)
    wt = np.ones(p.shape[0]); wt[inl] = om
    return dict(sums=tot, abs_sums=np.abs(T).sum(0), valid=int(ok.sum()), inliers=int(inl.sum()), q=q, r=r, valid_mask=ok, inlier_mask=inl, usable=usable, weight=wt)


def track(grid, depth, intr, dist, pose6, desc=None, order="numpy", trace=False):
    """i3d_track_frame_sdf.  pose6: world -> camera.  Returns (pose6, stats); stats has the fields of i3d_track_sdf_stats and, with trace=True, "trace" (per sums
    pass, the final one included), "steps" (|omega|, |upsilon| per solved step), "pivot", "points" (the sample array) and "index" (its pixels)."""
    d = default_desc() if desc is None else default_desc(**desc)
    pose6 = np.asarray(pose6, np.float64)
    pts, usable, idx = samples(depth, intr, dist, d["stride"], d["min_depth"], d["max_depth"])
    R, t = pose_to_cw(pose6)
    c = pivot(grid, pts, R, t)
    tp = np.array([t[a] - c[a] for a in range(3)])
    st = dict(iterations=0, status=1, valid_pixels=int(usable.sum()), valid=0, inliers=0, rms_initial=0.0, rms_final=0.0, min_pivot_ratio=0.0)
    tr, steps = [], []
    n_it, status = 0, 1
    for k in range(d["iterations"]):
        a = sums(grid, pts, R, tp, c, d["max_distance"], d["huber_delta"], order)
        tr.append(a)
        if k == 0:
            st["rms_initial"] = RT._rms(a["sums"])
        s, x, ratio = track_twin.solve(a["sums"])
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
    a = sums(grid, pts, R, tp, c, d["max_distance"], d["huber_delta"], order)
    tr.append(a)
    st.update(iterations=n_it, valid=a["valid"], inliers=a["inliers"], rms_final=RT._rms(a["sums"]))
    if d["iterations"] == 0:
        st["rms_initial"] = st["rms_final"]
        status = 2 if a["inliers"] < MIN_INLIERS else 1
    st["status"] = status
    if trace:
        st["trace"] = tr; st["steps"] = steps; st["pivot"] = c; st["points"] = pts; st["index"] = idx
    out = track_twin.cw_to_pose(R, np.array([tp[a_] + c[a_] for a_ in range(3)])) if n_it > 0 else pose6.copy()
    return out, st


def pose_err(a, b, vs):
    """two world -> camera poses: (angle between the rotations in rad, distance between the camera centres in voxels)"""
    Ra, ta = track_twin.pose_to_cw(np.asarray(a, np.float64)); Rb, tb = track_twin.pose_to_cw(np.asarray(b, np.float64))
    D = Ra @ Rb.T
    sk = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    ang = math.atan2(float(np.sqrt((sk * sk).sum())), 0.5 * (float(np.trace(D)) - 1.0))
    return ang, float(np.sqrt(((ta - tb) ** 2).sum())) / vs
