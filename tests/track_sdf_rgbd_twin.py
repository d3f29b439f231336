"""numpy statement of i3d_track_frame_sdf_rgbd, vectorised over the samples of the depth image, in fp64.

Test infrastructure: the device kernels (k_voxel_intensity and the PHOTO sums of track_sdf_kernels.hip, the step of track_kernels.hip) are compared against this.
Samples, points, pose, pivot, geometric residual, gate and Huber weight are track_sdf_twin's (section 19.1); on top of them the per-voxel intensity c and, for the
inliers, the photometric residual and row with the same fp64 expressions in the same order as the kernel.  Only the order of the sums over the samples differs
(numpy's here, or sequential with order="sequential").
"""
from __future__ import annotations

import math

import numpy as np

import query_twin
import register_twin as RT
import render_twin
import track_sdf_twin as ST
import track_twin

MIN_INLIERS = RT.MIN_INLIERS
UPPER = RT.UPPER
SUMS = 31                      # 21 upper-triangle J^T J | 6 J^T r (the combined system) | geometric r^2, count | photometric r^2, count
AXIS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.int64)      # NB_PX, NB_MX, NB_PY, NB_MY, NB_PZ, NB_MZ


def default_desc(**kw):
    """i3d_track_sdf_rgbd_desc_default (the camera is an argument of its own here)"""
    d = ST.default_desc(geometric_weight=1.0, photo_weight=0.1, max_photo_residual=0.0)
    d.update(kw)
    return d


def voxel_intensity(grid, with_terms=False):
    """section 21.1 item 1 on a render_twin.Grid with albedo and SH: c [N] in the grid's order, NaN where not defined; with_terms: also sum_j |alb sh_j| M_j [N],
    M_j the sum of the magnitudes of the parts of basis value j (so that a basis value that cancels still carries the rounding of its parts)"""
    g = grid
    nb = [g.find(g.keys + AXIS[i]) for i in range(6)]
    ok = g.weight != 0.0
    for n in nb:
        ok &= n >= 0
        ok &= g.weight[np.where(n >= 0, n, 0)] != 0.0
    F = [g.sdf[np.where(n >= 0, n, 0)] for n in nb]
    gx, gy, gz = F[0] - F[1], F[2] - F[3], F[4] - F[5]
    nl = np.sqrt((gx * gx + gy * gy) + gz * gz)
    with np.errstate(invalid="ignore"):
        ok &= nl > 0.0
    nls = np.where(ok, nl, 1.0)
    nx, ny, nz = gx / nls, gy / nls, gz / nls
    H = render_twin.sh_basis(nx, ny, nz)
    M = [np.ones_like(nx), np.abs(ny), np.abs(nz), np.abs(nx), np.abs(nx * ny), np.abs(ny * nz), nx * nx + ny * ny + 2.0 * nz * nz, np.abs(nx * nz), nx * nx + ny * ny]
    shade = np.zeros(g.keys.shape[0]); mag = np.zeros(g.keys.shape[0])
    for j in range(9):
        shade = shade + g.sh[:, j] * H[j]
        mag = mag + np.abs(g.sh[:, j]) * M[j]
    c = np.where(ok, g.alb * shade, np.nan)
    return (c, np.abs(g.alb) * mag) if with_terms else c


def luminance_samples(lum, idx):
    """the fp32 luminance of every sample, widened"""
    return np.asarray(lum, np.float32).reshape(-1)[idx].astype(np.float64)


def sums(grid, vol, pts, lum_s, R, tp, c, max_distance, huber_delta=0.0, wg=1.0, wp=0.1, max_photo_residual=0.0, order="numpy"):
    """one pass of k_track_sdf with PHOTO at the camera -> world pose (R, t' = t - c) about the pivot c.  vol: voxel_intensity(grid), or None when wp = 0 (no photometric
    block).  lum_s [n]: luminance_samples.  Returns dict(sums [31], abs_sums [31], valid, inliers, samples, q, r, valid_mask, inlier_mask, photo_mask [n],
    rp [n] (0 where there is no photometric sample before the gate), rp_mask [n] (samples whose r_p was formed, gate not yet applied))"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    n = p.shape[0]
    vs = grid.vs
    wg2, wp2 = wg * wg, wp * wp
    with np.errstate(invalid="ignore", over="ignore"):
        xp = RT._place(R, tp, p)
        x = np.stack([xp[:, a] + c[a] for a in range(3)], -1)
    ok, cidx, v, fr, q = query_twin._locate(grid, x)
    w = query_twin._weights(fr)
    r = np.where(ok, query_twin._tri(w, v), 0.0)
    gr, _ = query_twin._gradient(v, fr)
    inl = ok & (np.abs(r) <= max_distance)
    xi, ri = xp[inl], r[inl]
    d = [gr[inl][:, a] / vs for a in range(3)]
    J = [xi[:, 1] * d[2] - xi[:, 2] * d[1], xi[:, 2] * d[0] - xi[:, 0] * d[2], xi[:, 0] * d[1] - xi[:, 1] * d[0], d[0], d[1], d[2]]
    if huber_delta > 0.0:
        ar = np.abs(ri)
        with np.errstate(divide="ignore", invalid="ignore"):
            om = np.where(ar <= huber_delta, 1.0, huber_delta / ar)
        G = [wg2 * (om * (J[a] * J[b])) for a, b in UPPER] + [wg2 * (om * (J[a] * ri)) for a in range(6)]
    else:
        G = [wg2 * (J[a] * J[b]) for a, b in UPPER] + [wg2 * (J[a] * ri) for a in range(6)]
    m = ri.size
    ps = np.zeros(m, bool); rp = np.zeros(m); formed = np.zeros(m, bool)
    P = [np.zeros(m) for _ in range(27)]
    if vol is not None and wp > 0.0:
        cv = vol[cidx[inl]]
        li = lum_s[inl]
        formed = np.isfinite(cv).all(1) & np.isfinite(li)
        cvs = np.where(formed[:, None], cv, 0.0); lis = np.where(formed, li, 0.0)
        wi = [wk[inl] for wk in w]
        rp = np.where(formed, query_twin._tri(wi, cvs) - lis, 0.0)
        ps = formed & (np.abs(rp) <= max_photo_residual) if max_photo_residual > 0.0 else formed.copy()
        ge, _ = query_twin._gradient(cvs, fr[inl])
        e = [ge[:, a] / vs for a in range(3)]
        Jp = [xi[:, 1] * e[2] - xi[:, 2] * e[1], xi[:, 2] * e[0] - xi[:, 0] * e[2], xi[:, 0] * e[1] - xi[:, 1] * e[0], e[0], e[1], e[2]]
        P = [np.where(ps, wp2 * (Jp[a] * Jp[b]), 0.0) for a, b in UPPER] + [np.where(ps, wp2 * (Jp[a] * rp), 0.0) for a in range(6)]
    rps = np.where(ps, rp, 0.0)
    terms = [G[k] + P[k] for k in range(27)] + [ri * ri, np.ones_like(ri), rps * rps, ps.astype(np.float64)]
    mags = [np.abs(G[k]) + np.abs(P[k]) for k in range(27)] + [ri * ri, np.ones_like(ri), rps * rps, ps.astype(np.float64)]
    T = np.stack(terms, -1) if m else np.zeros((0, SUMS))
    A = np.stack(mags, -1) if m else np.zeros((0, SUMS))
    if order == "sequential":
        tot = np.zeros(SUMS)
        for row in T:
            tot = tot + row
    else:
        tot = np.ascontiguousarray(T.T).sum(1)
    def full(a, fill):
        o = np.full(n, fill, dtype=a.dtype); o[inl] = a
        return o
    return dict(sums=tot, abs_sums=A.sum(0), valid=int(ok.sum()), inliers=int(inl.sum()), samples=int(ps.sum()), q=q, r=r, valid_mask=ok, inlier_mask=inl,
                photo_mask=full(ps, False), rp=full(rp, 0.0), rp_mask=full(formed, False), usable=int(np.isfinite(p).all(1).sum()))


def solve(tot, wg):
    """k_track_solve on the combined system; the count that decides status 2 is the geometric one when wg > 0, else the photometric one"""
    t = np.array(tot[:29], np.float64)
    t[28] = tot[28] if wg > 0.0 else tot[30]
    return track_twin.solve(t)


def _rms(sq, n):
    return math.sqrt(sq / n) if n > 0 else 0.0


def track(grid, depth, lum, intr, dist, pose6, desc=None, order="numpy", trace=False):
    """i3d_track_frame_sdf_rgbd.  grid: a render_twin.Grid of the chosen field with albedo and SH (the SH may be missing when photo_weight = 0).  pose6: world ->
    camera.  Returns (pose6, stats); stats has the fields of i3d_track_sdf_rgbd_stats and, with trace=True, those of track_sdf_twin.track's trace."""
    d = default_desc() if desc is None else default_desc(**desc)
    wg, wp, gate = d["geometric_weight"], d["photo_weight"], d["max_photo_residual"]
    pose6 = np.asarray(pose6, np.float64)
    pts, usable, idx = ST.samples(depth, intr, dist, d["stride"], d["min_depth"], d["max_depth"])
    lum_s = luminance_samples(lum, idx)
    vol = voxel_intensity(grid) if wp > 0.0 else None
    R, t = ST.pose_to_cw(pose6)
    c = ST.pivot(grid, pts, R, t)
    tp = np.array([t[a] - c[a] for a in range(3)])
    st = dict(iterations=0, status=1, valid_pixels=int(usable.sum()), valid=0, inliers=0, rms_initial=0.0, rms_final=0.0, min_pivot_ratio=0.0, photo_samples=0,
              photo_rms_initial=0.0, photo_rms_final=0.0)
    one = lambda: sums(grid, vol, pts, lum_s, R, tp, c, d["max_distance"], d["huber_delta"], wg, wp, gate, order)  # noqa: E731
    tr, steps = [], []
    n_it, status = 0, 1
    for k in range(d["iterations"]):
        a = one()
        tr.append(a)
        if k == 0:
            st["rms_initial"] = _rms(a["sums"][27], a["sums"][28]); st["photo_rms_initial"] = _rms(a["sums"][29], a["sums"][30])
        s, x, ratio = solve(a["sums"], wg)
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


def photo_residual_at(grid, vol, pts, lum_s, R, tp, c):
    """r_p of every sample at the pose, NaN where there is none (no gate): for the derivative check"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        xp = RT._place(R, tp, p)
        x = np.stack([xp[:, a] + c[a] for a in range(3)], -1)
    ok, cidx, v, fr, q = query_twin._locate(grid, x)
    cv = vol[cidx]
    good = ok & np.isfinite(cv).all(1) & np.isfinite(lum_s)
    val = query_twin._tri(query_twin._weights(fr), np.where(good[:, None], cv, 0.0)) - np.where(good, lum_s, 0.0)
    return np.where(good, val, np.nan), np.floor(np.where(np.isfinite(q), q, 0.0)).astype(np.int64)


def photo_rows(grid, vol, pts, R, tp, c):
    """J_p [n, 6] of every sample at the pose (rows of samples without a valid cell are meaningless)"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        xp = RT._place(R, tp, p)
        x = np.stack([xp[:, a] + c[a] for a in range(3)], -1)
    ok, cidx, v, fr, q = query_twin._locate(grid, x)
    cv = np.where(np.isfinite(vol[cidx]), vol[cidx], 0.0)
    ge, _ = query_twin._gradient(cv, fr)
    e = [ge[:, a] / grid.vs for a in range(3)]
    return np.stack([xp[:, 1] * e[2] - xp[:, 2] * e[1], xp[:, 2] * e[0] - xp[:, 0] * e[2], xp[:, 0] * e[1] - xp[:, 1] * e[0], e[0], e[1], e[2]], -1)
