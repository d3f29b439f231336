"""numpy statement of the registration by depth and model intensity of i3d_track_frame_rgbd, vectorised over pixels, in fp64.

Test infrastructure: k_track_assoc_rgbd (track_kernels.hip) is compared against this.  Everything that section 16 leaves as section 14 comes from track_twin.py:
frame points, the association and its gates, the solve, the step.  What is stated here: the luminance pyramid, the photometric sample (bilinear interpolant of
the model's intensity plane and its derivative), the derivative of the forward camera model, the row J_p, the combined sums and the loop of levels and passes
with the model's intensity plane.  The expressions are those of the kernel in the same order (it is compiled without contraction); only the order of the big
sums differs.
"""
from __future__ import annotations

import math

import numpy as np

import track_twin
from track_twin import UPPER
from intrinsic3d_amd import synthetic

SUMS = 31                      # 21 upper-triangle J^T J | 6 J^T r (both weighted) | geometric r^2, count | photometric r^2, count


def pyr_down(img):
    """k_pyr_down (level_kernels.hip), the keyframes' luminance levels: the 5 x 5 [1 4 6 4 1] kernel with BORDER_REFLECT_101 in the kernel's fp32 operation
    order (synthetic.pyr_down is the same filter summed in another order, one fp32 rounding apart)"""
    I = np.asarray(img, np.float32)
    h, w = I.shape
    oh, ow = h // 2, w // 2

    def reflect(i, n):
        i = np.asarray(i)
        if n == 1:
            return np.zeros_like(i)
        for _ in range(4):
            i = np.where(i < 0, -i, i); i = np.where(i >= n, 2 * (n - 1) - i, i)
        return i

    f6, f4 = np.float32(6.0), np.float32(4.0)
    xs = [reflect(2 * np.arange(ow) + k, w) for k in (-2, -1, 0, 1, 2)]
    m2, m1, c0, p1, p2 = (I[:, x] for x in xs)
    rows = ((c0 * f6 + (m1 + p1) * f4) + m2) + p2                  # [h, ow]
    r = [rows[reflect(2 * np.arange(oh) + k, h)] for k in (-2, -1, 0, 1, 2)]
    return ((((r[2] * f6 + (r[1] + r[3]) * f4) + r[0]) + r[4]) * np.float32(1.0 / 256.0)).astype(np.float32)


def lum_pyramid(lum, levels):
    out = [np.asarray(lum, np.float32)]
    for _ in range(1, levels):
        out.append(pyr_down(out[-1]))
    return out


def project_jac(cam, q):
    """the forward model of observe_device.hpp (its y line reads the distorted x) at camera points q = (q0, q1, q2): (u, v) and d(xd, yd) / d(x, y) =
    (xx, xy, yx, yy) of the distortion, with x = q0 / q2, y = q1 / q2"""
    x = q[0] / q[2]; y = q[1] / q[2]
    k1, k2, k3, p1, p2 = cam["dist"]
    fx, fy, cx, cy = cam["intr"]
    if (np.abs(cam["dist"]) <= 1e-5).all():
        one, zero = np.ones_like(x), np.zeros_like(x)
        return fx * x + cx, fy * y + cy, x, y, (one, zero, zero, one)
    r2 = x * x + y * y; r4 = r2 * r2; r6 = r4 * r2
    dc = 1.0 + k1 * r2 + k2 * r4 + k3 * r6
    dr = (k1 + 2.0 * k2 * r2) + 3.0 * k3 * r4
    xd = x * dc + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * dc + 2.0 * p2 * xd * y + p1 * (r2 + 2.0 * y * y)
    xx = ((dc + x * (dr * (2.0 * x))) + 2.0 * p1 * y) + 6.0 * p2 * x
    xy = (x * (dr * (2.0 * y)) + 2.0 * p1 * x) + 2.0 * p2 * y
    yx = (y * (dr * (2.0 * x)) + 2.0 * p2 * (xx * y)) + 2.0 * p1 * x
    yy = ((dc + y * (dr * (2.0 * y))) + 2.0 * p2 * (xy * y + xd)) + 6.0 * p1 * y
    return fx * xd + cx, fy * yd + cy, x, y, (xx, xy, yx, yy)


def projection_jacobian(cam, q):
    """J_pi = d(u, v) / dq, [n, 2, 3]"""
    fx, fy = cam["intr"][0], cam["intr"][1]
    _, _, x, y, (xx, xy, yx, yy) = project_jac(cam, q)
    rows = []
    for hx, hy in ((fx * xx, fx * xy), (fy * yx, fy * yy)):
        rows.append(np.stack([hx / q[2], hy / q[2], -(hx * x + hy * y) / q[2]], -1))
    return np.stack(rows, 1)


def bilinear(img, us, vs):
    """the interpolant of section 16 item 3 at continuous coordinates inside the image: (value, d/du, d/dv), fp64 from the fp32 plane"""
    xf, yf = np.floor(us), np.floor(vs)
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    I = np.asarray(img, np.float32)
    I00 = I[y0, x0].astype(np.float64); I10 = I[y0, x0 + 1].astype(np.float64); I01 = I[y0 + 1, x0].astype(np.float64); I11 = I[y0 + 1, x0 + 1].astype(np.float64)
    fx, fy = us - xf, vs - yf
    gx, gy = 1.0 - fx, 1.0 - fy
    return gy * (gx * I00 + fx * I10) + fy * (gx * I01 + fx * I11), gy * (I10 - I00) + fy * (I11 - I01), gx * (I01 - I00) + fx * (I11 - I10)


def photometric(vtx, mask, mdepth, mintensity, lum, cam, ref, Rc, tc, max_distance, max_photo_residual=0.0):
    """the photometric samples of the geometric inliers `mask` [h*w]: dict(idx (pixels with a sample), r [n], J [n, 6])"""
    h, w = cam["h"], cam["w"]
    idx = np.nonzero(mask)[0]
    V = vtx.reshape(-1, 3).astype(np.float64)[idx]
    vx, vy, vz = V[:, 0], V[:, 1], V[:, 2]
    p = [((Rc[a, 0] * vx + Rc[a, 1] * vy) + Rc[a, 2] * vz) + tc[a] for a in range(3)]
    Rr, tr = ref["R"], ref["t"]
    q = [((Rr[a, 0] * p[0] + Rr[a, 1] * p[1]) + Rr[a, 2] * p[2]) + tr[a] for a in range(3)]
    u, v, x, y, (xx, xy, yx, yy) = project_jac(cam, q)
    ud, vd = u + 0.5, v + 0.5
    ui, vi = np.trunc(ud).astype(np.int64), np.trunc(vd).astype(np.int64)
    D = np.asarray(mdepth, np.float32)
    md = D[vi, ui].astype(np.float64)
    us, vs = ud - 0.5, vd - 0.5
    ur, vr = np.rint(us), np.rint(vs)                 # within 1e-9 pixel of a pixel centre: that centre, fraction 0 of the cell to its right / below
    us, vs = np.where(np.abs(us - ur) < 1e-9, ur, us), np.where(np.abs(vs - vr) < 1e-9, vr, vs)
    x0, y0 = np.floor(us).astype(np.int64), np.floor(vs).astype(np.int64)
    ok = (x0 >= 0) & (y0 >= 0) & (x0 + 1 < w) & (y0 + 1 < h)
    usc, vsc = np.where(ok, us, 0.0), np.where(ok, vs, 0.0)
    x0c, y0c = np.where(ok, x0, 0), np.where(ok, y0, 0)
    maxd = float(np.float32(max_distance))
    for dy in (0, 1):
        for dx in (0, 1):
            dk = D[y0c + dy, x0c + dx]
            ok &= (dk > 0) & (np.abs(dk.astype(np.float64) - md) <= maxd)
    Im, gu, gv = bilinear(mintensity, usc, vsc)
    rp = Im - np.asarray(lum, np.float32).ravel()[idx].astype(np.float64)
    mr = float(np.float32(max_photo_residual))
    if mr > 0.0:
        ok &= np.abs(rp) <= mr
    fx, fy = cam["intr"][0], cam["intr"][1]
    hx = gu * (fx * xx) + gv * (fy * yx); hy = gu * (fx * xy) + gv * (fy * yy)
    gq = [hx / q[2], hy / q[2], -(hx * x + hy * y) / q[2]]
    a = [(Rr[0, k] * gq[0] + Rr[1, k] * gq[1]) + Rr[2, k] * gq[2] for k in range(3)]
    J = [p[1] * a[2] - p[2] * a[1], p[2] * a[0] - p[0] * a[2], p[0] * a[1] - p[1] * a[0], a[0], a[1], a[2]]
    return dict(idx=idx[ok], r=rp[ok], J=np.stack(J, -1)[ok])


def associate_rgbd(vtx, nrm, mdepth, mnormal, mintensity, lum, cam, ref, Rc, tc, max_distance, min_normal_dot, wg, wp, max_photo_residual=0.0):
    """k_track_assoc_rgbd: dict(sums [31], abs_sums [31], valid, inliers, samples).  mintensity None or wp == 0: no photometric term."""
    g = track_twin.associate(vtx, nrm, mdepth, mnormal, cam, ref, Rc, tc, max_distance, min_normal_dot)
    wg2, wp2 = wg * wg, wp * wp
    sums = np.zeros(SUMS); abs_sums = np.zeros(SUMS)
    sums[:27] = wg2 * g["sums"][:27]; abs_sums[:27] = wg2 * g["abs_sums"][:27]
    sums[27:29] = g["sums"][27:29]; abs_sums[27:29] = g["abs_sums"][27:29]
    samples = 0
    if mintensity is not None and wp > 0.0:
        ph = photometric(vtx, g["mask"], mdepth, mintensity, lum, cam, ref, Rc, tc, max_distance, max_photo_residual)
        J, r = ph["J"], ph["r"]
        terms = [wp2 * (J[:, a] * J[:, b]) for a, b in UPPER] + [wp2 * (J[:, a] * r) for a in range(6)]
        T = np.stack(terms, -1) if len(r) else np.zeros((0, 27))
        sums[:27] += T.sum(0); abs_sums[:27] += np.abs(T).sum(0)
        sums[29] = abs_sums[29] = float((r * r).sum()); sums[30] = abs_sums[30] = float(len(r))
        samples = len(r)
    return dict(sums=sums, abs_sums=abs_sums, valid=g["valid"], inliers=g["inliers"], samples=samples)


def _solve(sums, wg):
    """k_track_solve on the combined system; the count that decides status 2 is the geometric one when wg > 0, else the photometric one"""
    tot = np.array(sums[:29], np.float64)
    tot[28] = sums[28] if wg > 0.0 else sums[30]
    return track_twin.solve(tot)


def _rms(sq, n):
    return math.sqrt(sq / n) if n > 0 else 0.0


def track_rgbd(depth, lum, intr, dist, pose6, model_fn, desc=None, wg=1.0, wp=0.1, max_photo_residual=0.0, trace=False):
    """i3d_track_frame_rgbd.  model_fn(level, cam, ref) -> (model depth [h, w], world normal [h, w, 3], intensity [h, w]) ray-cast at ref.  The loop of
    track_twin.track with the combined system.  Returns (pose6, stats); with `trace` (pose6, stats, passes), the records of track_twin.track with the 31 sums and
    `samples` (the photometric count of the pass's first association)"""
    passes = []
    d = track_twin.default_desc() if desc is None else desc
    h0, w0 = np.asarray(depth).shape
    pyr = track_twin.depth_pyramid(depth, d["levels"]); lpyr = lum_pyramid(lum, d["levels"])
    Rc, tc = track_twin.pose_to_cw(pose6)
    stats = dict(iterations=[0, 0, 0, 0], status=1, rms_initial=0.0, rms_final=0.0, min_pivot_ratio=0.0, valid_pixels=0, inliers=0, photo_samples=0,
                 photo_rms_initial=0.0, photo_rms_final=0.0)

    def planes(lvl):
        cam = track_twin.level_camera(intr, dist, w0, h0, lvl)
        ref = track_twin.ref_from_cw(Rc, tc)
        md, mn, mi = model_fn(lvl, cam, ref)
        passes.append(track_twin._pass_record(lvl, Rc, tc, ref))
        return (cam, ref, md, mn, mi) + track_twin.frame_points(pyr[lvl], cam, d["min_depth"], d["max_depth"])

    def assoc(pl, lvl):
        cam, ref, md, mn, mi, vtx, nrm = pl
        return associate_rgbd(vtx, nrm, md, mn, mi, lpyr[lvl], cam, ref, Rc, tc, d["max_distance"], d["min_normal_dot"], wg, wp, max_photo_residual)

    planes0 = None
    for lvl in range(d["levels"] - 1, -1, -1):
        budget = d["iterations"][lvl]
        if budget == 0 and lvl > 0:
            continue
        if budget == 0:
            planes0 = planes(0)
            break
        used, level_status, first_pass = 0, 1, True
        while used < budget:
            pl = planes(lvl)
            if lvl == 0:
                planes0 = pl
            status, n_it = 1, 0
            rec = passes[-1]
            for _ in range(budget - used):
                a = assoc(pl, lvl)
                if rec["sums"] is None:
                    rec.update(sums=a["sums"].copy(), inliers=a["inliers"], samples=a["samples"])
                if n_it == 0 and lvl == 0 and first_pass:
                    stats["rms_initial"] = _rms(a["sums"][27], a["sums"][28]); stats["photo_rms_initial"] = _rms(a["sums"][29], a["sums"][30])
                first_pass = False
                st, x, ratio = _solve(a["sums"], wg)
                if st == 2:
                    stats.update(status=2, valid_pixels=a["valid"], inliers=a["inliers"], photo_samples=a["samples"])
                    stats["iterations"][lvl] = used + n_it
                    rec.update(iterations=n_it, status=2)
                    out = np.asarray(pose6, np.float64).copy()
                    return (out, stats, passes) if trace else (out, stats)
                stats["min_pivot_ratio"] = ratio
                if st == 3:
                    status = 3
                    break
                Rc, tc = track_twin.apply_step(Rc, tc, x)
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
        planes0 = planes(0)
    a = assoc(planes0, 0)
    stats.update(valid_pixels=a["valid"], inliers=a["inliers"], photo_samples=a["samples"], rms_final=_rms(a["sums"][27], a["sums"][28]),
                 photo_rms_final=_rms(a["sums"][29], a["sums"][30]))
    out = track_twin.cw_to_pose(Rc, tc)
    return (out, stats, passes) if trace else (out, stats)


def orbit(pose, centre, rng, rot_deg, trans):
    """pose (world->camera) with its camera orbited by rot_deg about a seeded axis through `centre` (the motion a sphere's depth cannot see), then its centre
    moved by `trans` in a seeded direction"""
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    dt = rng.normal(size=3); dt *= trans / np.linalg.norm(dt)
    Q = synthetic.aa_to_rotmat(ax * math.radians(rot_deg))
    R = synthetic.aa_to_rotmat(np.asarray(pose[:3], np.float64)); c = -R.T @ np.asarray(pose[3:], np.float64)
    R2 = R @ Q.T                                   # the camera frame turns with the orbit: the sphere's depth image is unchanged
    c2 = np.asarray(centre, np.float64) + Q @ (c - centre) + dt
    return np.concatenate([synthetic.rotmat_to_aa(R2), -R2 @ c2])


# ---- the twin's own derivatives against central differences ---------------------------------------------------------------------------------------------------

def check_projection_jacobian(cam, q, h=1e-6):
    """max |J_pi - central difference| / max |J_pi| over the camera points q [n, 3]"""
    q = np.asarray(q, np.float64)
    J = projection_jacobian(cam, [q[:, 0], q[:, 1], q[:, 2]])
    N = np.zeros_like(J)
    for k in range(3):
        qa, qb = q.copy(), q.copy()
        qa[:, k] += h; qb[:, k] -= h
        ua, va = project_jac(cam, [qa[:, 0], qa[:, 1], qa[:, 2]])[:2]
        ub, vb = project_jac(cam, [qb[:, 0], qb[:, 1], qb[:, 2]])[:2]
        N[:, 0, k] = (ua - ub) / (2 * h); N[:, 1, k] = (va - vb) / (2 * h)
    return float(np.abs(J - N).max() / np.abs(J).max())


def check_photo_rows(vtx, mask, mdepth, mintensity, lum, cam, ref, Rc, tc, max_distance, h=1e-7, border=0.05):
    """max |J_p - central difference of r_p along each of the six step directions| / max |J_p| over the samples that stay inside their bilinear cell"""
    base = photometric(vtx, mask, mdepth, mintensity, lum, cam, ref, Rc, tc, max_distance)
    keep = np.zeros(mask.shape[0], bool); keep[base["idx"]] = True

    def coords(Rc_, tc_):                           # (us, vs, r_p with the interpolant of the unperturbed cell) of the pixels in `keep`
        V = vtx.reshape(-1, 3).astype(np.float64)[keep]
        p = [((Rc_[a, 0] * V[:, 0] + Rc_[a, 1] * V[:, 1]) + Rc_[a, 2] * V[:, 2]) + tc_[a] for a in range(3)]
        q = [((ref["R"][a, 0] * p[0] + ref["R"][a, 1] * p[1]) + ref["R"][a, 2] * p[2]) + ref["t"][a] for a in range(3)]
        u, v = project_jac(cam, q)[:2]
        return u, v

    u0, v0 = coords(Rc, tc)
    inner = (np.minimum(u0 - np.floor(u0), np.ceil(u0) - u0) > border) & (np.minimum(v0 - np.floor(v0), np.ceil(v0) - v0) > border)
    N = np.zeros((int(keep.sum()), 6))
    lumv = np.asarray(lum, np.float32).ravel()[keep].astype(np.float64)
    for k in range(6):
        x = np.zeros(6); x[k] = h
        ra = bilinear(mintensity, *coords(*track_twin.apply_step(Rc, tc, x)))[0] - lumv
        rb = bilinear(mintensity, *coords(*track_twin.apply_step(Rc, tc, -x)))[0] - lumv
        N[:, k] = (ra - rb) / (2 * h)
    J = base["J"]
    return float(np.abs(J - N)[inner].max() / np.abs(J).max()), int(inner.sum())
