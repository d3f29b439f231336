"""numpy statement of the frame registration of i3d_track_frame, vectorised over pixels, in fp64.

Test infrastructure: the device kernels (track_kernels.hip) are compared against this.  Frame points, association, residuals and Jacobians are the same fp64
expressions in the same order as the kernels (compiled without contraction); the solve is the same scalar fp64 code.  Only the order of the big sums differs
(the device sums in a fixed tree), so sums agree to rounding relative to the sum of the absolute values of their terms.
Poses: `pose6` is world->camera (angle-axis | t); the loop carries camera->world (Rc, tc), p = Rc v + tc.
"""
from __future__ import annotations

import math

import numpy as np

from intrinsic3d_amd import synthetic

SUMS = 29                      # 21 upper-triangle J^T J | 6 J^T r | r^2 | count
MIN_INLIERS = 64               # track_kernels.hpp TRACK_MIN_INLIERS
UPPER = [(a, b) for a in range(6) for b in range(a, 6)]


def default_desc(**kw):
    """i3d_track_desc_default"""
    d = dict(levels=1, iterations=[30, 10, 10, 10], max_distance=0.05, min_normal_dot=0.8, min_depth=0.0, max_depth=0.0,
             stop_rotation=1e-6, stop_translation=1e-6)
    d.update(kw)
    return d


def level_camera(intr, dist, w, h, level):
    """intrinsics x 2^-level (all four, as make_params), the level size of set_frames_rgbd (halved `level` times, rounding down)"""
    s = 1.0 / math.pow(2.0, level)
    for _ in range(level):
        w, h = w // 2, h // 2
    return dict(intr=np.asarray(intr, np.float64) * s, dist=np.asarray(dist, np.float64), w=int(w), h=int(h))


def depth_pyramid(depth, levels):
    out = [np.asarray(depth, np.float32)]
    for _ in range(1, levels):
        out.append(synthetic.depth_down(out[-1]))
    return out


def undistort(cam, u, v):
    """the renderer's ray of the integer pixel (u, v): 10 fixed-point iterations of the inverse of observe_device.hpp's forward model"""
    fx, fy, cx, cy = cam["intr"]
    xd = (u - cx) / fx; yd = (v - cy) / fy
    x, y = xd.copy(), yd.copy()
    k1, k2, k3, p1, p2 = cam["dist"]
    if not (np.abs(cam["dist"]) <= 1e-5).all():
        for _ in range(10):
            r2 = x * x + y * y; r4 = r2 * r2; r6 = r4 * r2
            dc = 1.0 + k1 * r2 + k2 * r4 + k3 * r6
            xn = (xd - (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) / dc
            yn = (yd - (2.0 * p2 * xd * y + p1 * (r2 + 2.0 * y * y))) / dc
            x, y = xn, yn
    return x, y


def frame_points(depth, cam, min_depth=0.0, max_depth=0.0):
    """k_track_points: fp32 vertex and normal planes [h, w, 3] in the camera frame; invalid pixels are all zero"""
    z = np.asarray(depth, np.float32)
    h, w = z.shape
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ok = z > 0
    if min_depth > 0:
        ok &= ~(z < np.float32(min_depth))
    if max_depth > 0:
        ok &= ~(z > np.float32(max_depth))
    x, y = undistort(cam, u, v)
    zd = z.astype(np.float64)
    P = np.stack([x * zd, y * zd, zd], -1)
    okr = np.zeros_like(ok); okr[:, :-1] = ok[:, 1:]
    okd = np.zeros_like(ok); okd[:-1, :] = ok[1:, :]
    valid = ok & okr & okd
    Pr = np.zeros_like(P); Pr[:, :-1] = P[:, 1:]
    Pd = np.zeros_like(P); Pd[:-1, :] = P[1:, :]
    a = Pr - P; b = Pd - P
    nx = b[..., 1] * a[..., 2] - b[..., 2] * a[..., 1]
    ny = b[..., 2] * a[..., 0] - b[..., 0] * a[..., 2]
    nz = b[..., 0] * a[..., 1] - b[..., 1] * a[..., 0]
    nl = np.sqrt((nx * nx + ny * ny) + nz * nz)
    valid &= nl > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        n = np.stack([nx / nl, ny / nl, nz / nl], -1)
    vtx = np.where(valid[..., None], P, 0.0).astype(np.float32)
    nrm = np.where(valid[..., None], n, 0.0).astype(np.float32)
    return vtx, nrm


def pose_to_cw(pose6):
    """world->camera (angle-axis | t) -> camera->world (Rc, tc)"""
    R = synthetic.aa_to_rotmat(np.asarray(pose6[:3], np.float64))
    t = np.asarray(pose6[3:], np.float64)
    tc = np.array([-((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2]) for a in range(3)])
    return R.T.copy(), tc


def cw_to_pose(Rc, tc):
    R = Rc.T
    t = np.array([-((R[a, 0] * tc[0] + R[a, 1] * tc[1]) + R[a, 2] * tc[2]) for a in range(3)])
    return np.concatenate([synthetic.rotmat_to_aa(R), t])


def ref_from_cw(Rc, tc):
    """the ray cast's camera: R world->camera, t, eye"""
    R = Rc.T.copy()
    t = np.array([-((R[a, 0] * tc[0] + R[a, 1] * tc[1]) + R[a, 2] * tc[2]) for a in range(3)])
    return dict(R=R, t=t, eye=np.asarray(tc, np.float64).copy())


def ref_from_pose(pose6):
    R = synthetic.aa_to_rotmat(np.asarray(pose6[:3], np.float64))
    t = np.asarray(pose6[3:], np.float64)
    eye = np.array([-((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2]) for a in range(3)])
    return dict(R=R, t=t.copy(), eye=eye)


def associate(vtx, nrm, mdepth, mnormal, cam, ref, Rc, tc, max_distance, min_normal_dot):
    """k_track_assoc: returns dict(sums [29], abs_sums [29], valid, inliers, mask [h*w] of the inliers)"""
    V = vtx.reshape(-1, 3).astype(np.float64); Nv = nrm.reshape(-1, 3).astype(np.float64)
    h, w = cam["h"], cam["w"]
    valid = V[:, 2] > 0
    vx, vy, vz = V[:, 0], V[:, 1], V[:, 2]
    p = [((Rc[a, 0] * vx + Rc[a, 1] * vy) + Rc[a, 2] * vz) + tc[a] for a in range(3)]
    Rr, tr = ref["R"], ref["t"]
    q = [((Rr[a, 0] * p[0] + Rr[a, 1] * p[1]) + Rr[a, 2] * p[2]) + tr[a] for a in range(3)]
    inn = valid & (q[2] > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = q[0] / q[2]; y = q[1] / q[2]
        k1, k2, k3, p1, p2 = cam["dist"]
        if not (np.abs(cam["dist"]) <= 1e-5).all():
            r2 = x * x + y * y; r4 = r2 * r2; r6 = r4 * r2
            dc = 1.0 + k1 * r2 + k2 * r4 + k3 * r6
            x = x * dc + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
            y = y * dc + 2.0 * p2 * x * y + p1 * (r2 + 2.0 * y * y)
        fx, fy, cx, cy = cam["intr"]
        ud = (fx * x + cx) + 0.5; vd = (fy * y + cy) + 0.5
        inn &= (ud > -1.0) & (ud < w) & (vd > -1.0) & (vd < h)
    ui = np.trunc(np.where(inn, ud, 0.0)).astype(np.int64); vi = np.trunc(np.where(inn, vd, 0.0)).astype(np.int64)
    md = np.where(inn, np.asarray(mdepth, np.float32)[vi, ui], np.float32(0))
    hit = md > 0
    nm = np.asarray(mnormal, np.float32)[vi, ui].astype(np.float64)
    rx, ry = undistort(cam, ui.astype(np.float64), vi.astype(np.float64))
    m = [ref["eye"][a] + md.astype(np.float64) * ((Rr[0, a] * rx + Rr[1, a] * ry) + Rr[2, a]) for a in range(3)]
    dx, dy, dz = p[0] - m[0], p[1] - m[1], p[2] - m[2]
    d2 = (dx * dx + dy * dy) + dz * dz
    nw = [(Rc[a, 0] * Nv[:, 0] + Rc[a, 1] * Nv[:, 1]) + Rc[a, 2] * Nv[:, 2] for a in range(3)]
    dot = (nm[:, 0] * nw[0] + nm[:, 1] * nw[1]) + nm[:, 2] * nw[2]
    maxd = float(np.float32(max_distance))
    inl = hit & ((nm[:, 0] != 0) | (nm[:, 1] != 0) | (nm[:, 2] != 0)) & (d2 <= maxd * maxd) & (dot >= float(np.float32(min_normal_dot)))
    r = (nm[:, 0] * dx + nm[:, 1] * dy) + nm[:, 2] * dz
    J = [p[1] * nm[:, 2] - p[2] * nm[:, 1], p[2] * nm[:, 0] - p[0] * nm[:, 2], p[0] * nm[:, 1] - p[1] * nm[:, 0], nm[:, 0], nm[:, 1], nm[:, 2]]
    terms = [J[a] * J[b] for a, b in UPPER] + [J[a] * r for a in range(6)] + [r * r, np.ones_like(r)]
    T = np.stack([t[inl] for t in terms], -1)
    return dict(sums=T.sum(0), abs_sums=np.abs(T).sum(0), valid=int(valid.sum()), inliers=int(inl.sum()), mask=inl)


def rodrigues(w):
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = math.sqrt(th2)
    if not th2 > 0.0:
        return np.eye(3)
    k0, k1, k2 = w[0] / th, w[1] / th, w[2] / th
    co, si = math.cos(th), math.sin(th)
    v = 1.0 - co
    return np.array([[co + k0 * k0 * v, k0 * k1 * v - k2 * si, k0 * k2 * v + k1 * si],
                     [k1 * k0 * v + k2 * si, co + k1 * k1 * v, k1 * k2 * v - k0 * si],
                     [k2 * k0 * v - k1 * si, k2 * k1 * v + k0 * si, co + k2 * k2 * v]])


def _fmax(a, b):
    """C's fmax: a NaN argument is ignored"""
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def solve(tot):
    """k_track_solve's factorisation: returns (status None | 2 | 3, delta (omega, upsilon), min / max pivot).  The factorisation stops at the first pivot that
    fails d > 1e-12 trace: status 3, ratio = max(d, 0) / (largest pivot up to and including that column if > 0, else ratio 0)"""
    tot = [float(x) for x in tot]
    if tot[28] < MIN_INLIERS:
        return 2, None, 0.0
    A = [[0.0] * 6 for _ in range(6)]
    for k, (a, c) in enumerate(UPPER):
        A[a][c] = A[c][a] = tot[k]
    b = tot[21:27]
    trace = A[0][0]
    for a in range(1, 6):
        trace = trace + A[a][a]
    L = [[0.0] * 6 for _ in range(6)]
    piv = [0.0] * 6
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        piv[j] = d
        if not d > 1e-12 * trace:
            pm = piv[0]
            for k in range(1, j + 1):
                pm = _fmax(pm, piv[k])
            return 3, None, (_fmax(d, 0.0) / pm if pm > 0.0 else 0.0)
        L[j][j] = math.sqrt(max(d, 0.0))
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j] if L[j][j] != 0.0 else math.inf
    ratio = min(piv) / max(piv) if max(piv) > 0 else 0.0
    y = [0.0] * 6
    for i in range(6):
        v = -b[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v / L[i][i]
    x = [0.0] * 6
    for i in range(5, -1, -1):
        v = y[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v / L[i][i]
    return None, np.array(x), ratio


def apply_step(Rc, tc, x):
    """T_cw <- exp(delta) T_cw, exp(omega, upsilon): p -> R(omega) p + upsilon"""
    Rd = rodrigues(x[:3])
    Rn = np.array([[(Rd[a, 0] * Rc[0, c] + Rd[a, 1] * Rc[1, c]) + Rd[a, 2] * Rc[2, c] for c in range(3)] for a in range(3)])
    tn = np.array([((Rd[a, 0] * tc[0] + Rd[a, 1] * tc[1]) + Rd[a, 2] * tc[2]) + x[3 + a] for a in range(3)])
    return Rn, tn


def track(depth, intr, dist, pose6, model_fn, desc=None, trace=False):
    """i3d_track_frame.  model_fn(level, cam, ref) -> (model depth [h, w], model world normal [h, w, 3]) ray-cast at ref.  Returns (pose6, stats); with `trace`
    (pose6, stats, passes): one record per pass in order, dict(level, pose (the cast's, world->camera), R, t, eye (the cast's camera), iterations, status
    (0 | 1 | 2 | 3), steps [(|omega|, |upsilon|) of every solved step], sums (the pass's first association), inliers (of that association)); a level-0 cast
    taken for the final figures only (budget 0, or after a degenerate coarser level) is a record with iterations 0, status None and sums None"""
    passes = []
    d = default_desc() if desc is None else desc
    h0, w0 = np.asarray(depth).shape
    pyr = depth_pyramid(depth, d["levels"])
    Rc, tc = pose_to_cw(pose6)
    stats = dict(iterations=[0, 0, 0, 0], status=1, rms_initial=0.0, rms_final=0.0, min_pivot_ratio=0.0, valid_pixels=0, inliers=0)
    planes0 = None
    for lvl in range(d["levels"] - 1, -1, -1):
        budget = d["iterations"][lvl]
        if budget == 0 and lvl > 0:
            continue
        cam = level_camera(intr, dist, w0, h0, lvl)
        if budget == 0:
            ref = ref_from_cw(Rc, tc)
            md, mn = model_fn(lvl, cam, ref)
            planes0 = (cam, ref, md, mn) + frame_points(pyr[0], cam, d["min_depth"], d["max_depth"])
            passes.append(_pass_record(0, Rc, tc, ref))
            break
        used, level_status, first_pass = 0, 1, True
        while used < budget:                    # passes: a fresh ray cast at the current pose each
            ref = ref_from_cw(Rc, tc)
            md, mn = model_fn(lvl, cam, ref)
            vtx, nrm = frame_points(pyr[lvl], cam, d["min_depth"], d["max_depth"])
            if lvl == 0:
                planes0 = (cam, ref, md, mn, vtx, nrm)
            status, n_it = 1, 0
            rec = _pass_record(lvl, Rc, tc, ref)
            passes.append(rec)
            for _ in range(budget - used):
                a = associate(vtx, nrm, md, mn, cam, ref, Rc, tc, d["max_distance"], d["min_normal_dot"])
                if rec["sums"] is None:
                    rec.update(sums=a["sums"].copy(), inliers=a["inliers"])
                if n_it == 0 and status == 1 and lvl == 0 and first_pass:
                    cnt = a["sums"][28]
                    stats["rms_initial"] = math.sqrt(a["sums"][27] / cnt) if cnt > 0 else 0.0
                first_pass = False
                st, x, ratio = solve(a["sums"])
                if st == 2:
                    stats.update(status=2, valid_pixels=a["valid"], inliers=a["inliers"])
                    stats["iterations"][lvl] = used + n_it
                    rec.update(iterations=n_it, status=2)
                    out = np.asarray(pose6, np.float64).copy()
                    return (out, stats, passes) if trace else (out, stats)
                stats["min_pivot_ratio"] = ratio
                if st == 3:
                    status = 3
                    break
                Rc, tc = apply_step(Rc, tc, x)
                n_it += 1
                rec["steps"].append((math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), math.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5])))
                if math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) < d["stop_rotation"] and \
                   math.sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]) < d["stop_translation"]:
                    status = 0
                    break
            used += n_it
            stats["iterations"][lvl] = used
            level_status = status
            rec.update(iterations=n_it, status=status)
            if status != 0 or n_it <= 1:
                break
        stats["status"] = level_status
        if level_status == 3:
            break
    if planes0 is None:
        cam = level_camera(intr, dist, w0, h0, 0)
        ref = ref_from_cw(Rc, tc)
        md, mn = model_fn(0, cam, ref)
        vtx, nrm = frame_points(pyr[0], cam, d["min_depth"], d["max_depth"])
        planes0 = (cam, ref, md, mn, vtx, nrm)
        passes.append(_pass_record(0, Rc, tc, ref))
    cam, ref, md, mn, vtx, nrm = planes0
    a = associate(vtx, nrm, md, mn, cam, ref, Rc, tc, d["max_distance"], d["min_normal_dot"])
    stats.update(valid_pixels=a["valid"], inliers=a["inliers"], rms_final=math.sqrt(a["sums"][27] / a["sums"][28]) if a["sums"][28] > 0 else 0.0)
    out = cw_to_pose(Rc, tc)
    return (out, stats, passes) if trace else (out, stats)


def _pass_record(lvl, Rc, tc, ref):
    return dict(level=lvl, pose=cw_to_pose(Rc, tc), R=ref["R"].copy(), t=ref["t"].copy(), eye=ref["eye"].copy(), iterations=0, status=None, steps=[], sums=None,
                inliers=0)


def rot_err_deg(p, q):
    R = synthetic.aa_to_rotmat(p[:3]) @ synthetic.aa_to_rotmat(q[:3]).T
    return math.degrees(math.acos(min(1.0, max(-1.0, (np.trace(R) - 1.0) * 0.5))))


def centre_err(p, q):
    c = lambda x: -synthetic.aa_to_rotmat(x[:3]).T @ x[3:]
    return float(np.linalg.norm(c(p) - c(q)))


def perturb(pose, rng, rot_deg, trans):
    """pose (world->camera) with its camera rotated by rot_deg about a random axis and its centre moved by `trans` in a random direction"""
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    dt = rng.normal(size=3); dt *= trans / np.linalg.norm(dt)
    R = synthetic.aa_to_rotmat(pose[:3]); c = -R.T @ pose[3:]
    R2 = synthetic.aa_to_rotmat(ax * math.radians(rot_deg)) @ R
    c2 = c + dt
    return np.concatenate([synthetic.rotmat_to_aa(R2), -R2 @ c2])


def raycast_scene(scene, cam, ref, iters=200, max_t=None):
    """analytic model planes: the bumpy sphere's SDF marched along the renderer's rays (damped sphere tracing), normals of the analytic field"""
    h, w = cam["h"], cam["w"]
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    x, y = undistort(cam, u.ravel(), v.ravel())
    R = ref["R"]
    d = np.stack([(R[0, a] * x + R[1, a] * y) + R[2, a] for a in range(3)], -1)
    dl = np.linalg.norm(d, axis=1)
    oc = ref["eye"] - scene.c
    a_ = (d * d).sum(1); b_ = 2.0 * (d @ oc); c_ = oc @ oc - (scene.R + 2 * abs(scene.amp)) ** 2
    disc = b_ * b_ - 4 * a_ * c_
    near = np.where(disc > 0, (-b_ - np.sqrt(np.maximum(disc, 0))) / (2 * a_), np.inf)
    t = np.where(np.isfinite(near), np.maximum(near, 0.0), 0.0)
    live = np.isfinite(near)
    lip = 1.0 + abs(scene.amp) * scene.freq * math.sqrt(3.0)
    for _ in range(iters):
        f = scene.sdf(ref["eye"] + t[:, None] * d)
        t = np.where(live, t + 0.9 * f / (lip * dl), t)
    p = ref["eye"] + t[:, None] * d
    f = scene.sdf(p)
    hit = live & (np.abs(f) < 1e-9)
    depth = np.where(hit, t, 0.0).astype(np.float32).reshape(h, w)
    n = scene.normal(p)
    normal = np.where(hit[:, None], n, 0.0).astype(np.float32).reshape(h, w, 3)
    return depth, normal
