"""numpy statement of i3d_register_points, vectorised over points, in fp64.

Test infrastructure: the device kernels (register_kernels.hip, the step of track_kernels.hip) are compared against this.  It places the points, evaluates the
cell of query_twin.py and forms the residual and the Jacobian with the same fp64 expressions in the same order as the kernel (which is compiled without
contraction); the 6x6 step is track_twin.solve / apply_step, the statement of k_track_solve.  Only the order of the sums over the points differs (numpy's here,
or sequential with order="sequential"), so per-point terms agree to the bit and every discrete decision (cell, inlier, stop) is the same unless a placed point
sits on a cell face, a residual on the gate or a step on the stop rule.
"""
from __future__ import annotations

import math

import numpy as np

import query_twin
import track_twin
from intrinsic3d_amd import synthetic

MIN_INLIERS = track_twin.MIN_INLIERS
UPPER = track_twin.UPPER


def default_desc(**kw):
    d = dict(iterations=30, max_distance=0.05, stop_rotation=1e-6, stop_translation=1e-6)
    d.update(kw)
    return d


def pose_to_rt(pose6):
    """angle-axis | t, points' frame -> world: (R, t)"""
    return synthetic.aa_to_rotmat(np.asarray(pose6[:3], np.float64)), np.asarray(pose6[3:], np.float64).copy()


def rt_to_pose(R, t):
    return np.concatenate([synthetic.rotmat_to_aa(R), t])


def _place(R, t, p):
    return np.stack([((R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1]) + R[a, 2] * p[:, 2]) + t[a] for a in range(3)], -1)


def counted(grid, points, R0, t0):
    """the points of the pivot mean: three finite coordinates, and R0 p + t0 finite with |x / vs| < 2^20 on every axis"""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        x = _place(R0, t0, p)
        return np.isfinite(p).all(1) & np.isfinite(x).all(1) & (np.abs(x / grid.vs) < query_twin.MAX_COORD).all(1)


def pivot(grid, points, pose6):
    """c = R0 mean(p) + t0 over the points that count (section 18.1 item 1)"""
    R0, t0 = pose_to_rt(pose6)
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    ok = counted(grid, p, R0, t0)
    m = p[ok].sum(0) / float(ok.sum()) if ok.any() else np.zeros(3)
    return np.array([((R0[a, 0] * m[0] + R0[a, 1] * m[1]) + R0[a, 2] * m[2]) + t0[a] for a in range(3)])


def sums(grid, points, R, tp, c, max_distance, order="numpy"):
    """one pass of k_register at the pose (R, t' = t - c) about the pivot c: dict(sums [29], abs_sums [29] (sum |term|), valid, inliers, q [n, 3] (the placed
    points in voxel units), r [n] (0 where not valid), valid_mask, inlier_mask)"""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    vs = grid.vs
    with np.errstate(invalid="ignore", over="ignore"):
        xp = _place(R, tp, p)
        x = np.stack([xp[:, a] + c[a] for a in range(3)], -1)
    ok, _, v, fr, q = query_twin._locate(grid, x)
    r = np.where(ok, query_twin._tri(query_twin._weights(fr), v), 0.0)
    gr, _ = query_twin._gradient(v, fr)
    inl = ok & (np.abs(r) <= max_distance)
    xi, ri = xp[inl], r[inl]
    d = [gr[inl][:, a] / vs for a in range(3)]
    J = [xi[:, 1] * d[2] - xi[:, 2] * d[1], xi[:, 2] * d[0] - xi[:, 0] * d[2], xi[:, 0] * d[1] - xi[:, 1] * d[0], d[0], d[1], d[2]]
    terms = [J[a] * J[b] for a, b in UPPER] + [J[a] * ri for a in range(6)] + [ri * ri, np.ones_like(ri)]
    T = np.stack(terms, -1) if ri.size else np.zeros((0, 29))
    if order == "sequential":
        tot = np.zeros(29)
        for row in T:
            tot = tot + row
    else:
        tot = np.ascontiguousarray(T.T).sum(1)         # numpy's pairwise sum along the contiguous axis (T.sum(0) would add the rows one after another)
    return dict(sums=tot, abs_sums=np.abs(T).sum(0), valid=int(ok.sum()), inliers=int(inl.sum()), q=q, r=r, valid_mask=ok, inlier_mask=inl)


def _rms(s):
    return math.sqrt(s[27] / s[28]) if s[28] > 0 else 0.0


def register(grid, points, pose6, desc=None, order="numpy", trace=False):
    """i3d_register_points.  Returns (pose6, stats); stats has the fields of i3d_register_stats and, with trace=True, "trace": per sums pass (the final one
    included) dict(q, r, valid_mask) and "steps": per solved step (|omega|, |upsilon|)."""
    d = default_desc() if desc is None else default_desc(**desc)
    pose6 = np.asarray(pose6, np.float64)
    R, t = pose_to_rt(pose6)
    c = pivot(grid, points, pose6)
    tp = np.array([t[a] - c[a] for a in range(3)])
    st = dict(iterations=0, status=1, valid=0, inliers=0, rms_initial=0.0, rms_final=0.0, min_pivot_ratio=0.0)
    tr, steps = [], []
    n_it, status = 0, 1
    for k in range(d["iterations"]):
        a = sums(grid, points, R, tp, c, d["max_distance"], order)
        tr.append(a)
        if k == 0:
            st["rms_initial"] = _rms(a["sums"])
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
    a = sums(grid, points, R, tp, c, d["max_distance"], order)
    tr.append(a)
    st.update(iterations=n_it, valid=a["valid"], inliers=a["inliers"], rms_final=_rms(a["sums"]))
    if d["iterations"] == 0:
        st["rms_initial"] = st["rms_final"]
        status = 2 if a["inliers"] < MIN_INLIERS else 1
    st["status"] = status
    if trace:
        st["trace"] = tr; st["steps"] = steps; st["pivot"] = c
    out = rt_to_pose(R, np.array([tp[a_] + c[a_] for a_ in range(3)])) if n_it > 0 else pose6.copy()
    return out, st


def pose_diff(a, b, vs):
    """(rotation angle between the two poses in rad, |t_a - t_b| in voxels)"""
    Ra, Rb = synthetic.aa_to_rotmat(np.asarray(a[:3], np.float64)), synthetic.aa_to_rotmat(np.asarray(b[:3], np.float64))
    D = Ra @ Rb.T
    sk = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    ang = math.atan2(float(np.sqrt((sk * sk).sum())), 0.5 * (float(np.trace(D)) - 1.0))
    return ang, float(np.sqrt(((np.asarray(a[3:], np.float64) - np.asarray(b[3:], np.float64)) ** 2).sum())) / vs
