"""numpy statement of the ray casting of i3d_render_view, vectorised over pixels, in fp64.

Test infrastructure: the device kernel (render_kernels.hip) is compared against this.  It evaluates the same fp64 expressions in the same order as the kernel
(which is compiled without contraction), so the two agree to rounding of the camera rotation, and any larger difference is a defect of one of them.
Inputs are the exported grid (visit order) and a camera given as (R world->camera, eye = camera centre in world, fx, fy, cx, cy, dist5, w, h).
"""
from __future__ import annotations

import numpy as np

MAX_SAMPLES = 1 << 14          # render_kernels.hpp RENDER_MAX_SAMPLES
BRICK_SHIFT = 3                # 8^3-voxel bricks
_B = 1 << 20


def pack(k):
    k = np.asarray(k, np.int64) + _B
    return (k[..., 0] & 0x1FFFFF) | ((k[..., 1] & 0x1FFFFF) << 21) | ((k[..., 2] & 0x1FFFFF) << 42)


def sh_basis(nx, ny, nz):
    """shading.h:53-67 (synthetic.sh_basis), in the kernel's operation order"""
    return [np.ones_like(nx), ny, nz, nx, nx * ny, ny * nz, -nx * nx - ny * ny + 2.0 * nz * nz, nx * nz, nx * nx - ny * ny]


class Grid:
    """The stored voxels with a sorted-key lookup and the brick bitmap of the voxels with weight != 0."""

    def __init__(self, keys, sdf, weight, voxel_size, albedo=None, sh=None):
        self.keys = np.asarray(keys, np.int64)
        self.sdf = np.asarray(sdf, np.float64)
        self.weight = np.asarray(weight, np.float32)
        self.alb = None if albedo is None else np.asarray(albedo, np.float64)
        self.sh = None if sh is None else np.asarray(sh, np.float64).astype(np.float32).astype(np.float64)     # the device keeps the SH in fp32
        self.vs = float(np.float32(voxel_size))
        p = pack(self.keys)
        self.order = np.argsort(p, kind="stable")
        self.sorted = p[self.order]
        on = self.weight != 0.0
        if on.any():
            br = self.keys[on] >> BRICK_SHIFT
            self.lo = br.min(0); self.dim = br.max(0) - self.lo + 1
            self.bits = np.zeros(self.dim[::-1], bool)                      # [z][y][x]
            rel = br - self.lo
            self.bits[rel[:, 2], rel[:, 1], rel[:, 0]] = True
        else:
            self.lo = np.zeros(3, np.int64); self.dim = np.zeros(3, np.int64); self.bits = np.zeros((0, 0, 0), bool)

    def find(self, k):
        p = pack(k)
        pos = np.minimum(np.searchsorted(self.sorted, p), len(self.sorted) - 1)
        return np.where(self.sorted[pos] == p, self.order[pos], -1)

    def cell(self, b):
        """corners [M, 8] (corner i = base + (i & 1, i >> 1 & 1, i >> 2)), values [M, 8], valid [M]: all corners stored with weight != 0"""
        off = np.array([[i & 1, (i >> 1) & 1, i >> 2] for i in range(8)], np.int64)
        c = self.find(b[:, None, :] + off[None, :, :])
        ok = (c >= 0).all(1)
        cc = np.where(c >= 0, c, 0)
        ok &= (self.weight[cc] != 0.0).all(1)
        return cc, self.sdf[cc], ok


def camera_from_pose(pose6, intr, dist, w, h):
    """R (world->camera), eye = -R^T t, scaled intrinsics as given"""
    from intrinsic3d_amd import synthetic
    R = synthetic.aa_to_rotmat(np.asarray(pose6[:3], np.float64))
    t = np.asarray(pose6[3:], np.float64)
    eye = np.array([-((R[0, a] * t[0] + R[1, a] * t[1]) + R[2, a] * t[2]) for a in range(3)])
    return dict(R=R, eye=eye, intr=np.asarray(intr, np.float64), dist=np.asarray(dist, np.float64), w=int(w), h=int(h))


def rays(cam):
    """per pixel (row-major): direction R^T (x, y, 1) with (x, y) the undistorted normalised coordinates of the integer pixel, and 1 / |direction|"""
    fx, fy, cx, cy = cam["intr"]
    v, u = np.meshgrid(np.arange(cam["h"], dtype=np.float64), np.arange(cam["w"], dtype=np.float64), indexing="ij")
    xd = ((u - cx) / fx).ravel(); yd = ((v - cy) / fy).ravel()
    x, y = xd.copy(), yd.copy()
    k1, k2, k3, p1, p2 = cam["dist"]
    if not (np.abs(cam["dist"]) <= 1e-5).all():
        for _ in range(10):
            r2 = x * x + y * y; r4 = r2 * r2; r6 = r4 * r2
            dc = 1.0 + k1 * r2 + k2 * r4 + k3 * r6
            xn = (xd - (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) / dc
            yn = (yd - (2.0 * p2 * xd * y + p1 * (r2 + 2.0 * y * y))) / dc
            x, y = xn, yn
    R = cam["R"]
    d = np.stack([(R[0, a] * x + R[1, a] * y) + R[2, a] for a in range(3)], -1)
    inv_len = 1.0 / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return d, inv_len


def project(cam, p):
    """the forward camera model of the observation pass (observe_device.hpp) in fp64: world points [M, 3] -> pixel coordinates (u, v)"""
    q = (p - cam["eye"]) @ cam["R"].T
    x, y = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
    k1, k2, k3, p1, p2 = cam["dist"]
    if not (np.abs(cam["dist"]) <= 1e-5).all():
        r2 = x * x + y * y; r4 = r2 * r2; r6 = r4 * r2
        dc = 1.0 + k1 * r2 + k2 * r4 + k3 * r6
        x = x * dc + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        y = y * dc + 2.0 * p2 * x * y + p1 * (r2 + 2.0 * y * y)
    fx, fy, cx, cy = cam["intr"]
    return fx * x + cx, fy * y + cy


def _weights(f):
    gx, gy, gz = 1.0 - f[:, 0], 1.0 - f[:, 1], 1.0 - f[:, 2]
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    return [gx * gy * gz, fx * gy * gz, gx * fy * gz, fx * fy * gz, gx * gy * fz, fx * gy * fz, gx * fy * fz, fx * fy * fz]


def _tri(w, v):
    s = w[0] * v[:, 0]
    for i in range(1, 8):
        s = s + w[i] * v[:, i]
    return s


def render(grid: Grid, cam, tmin=0.0, tmax=0.0, lum=None):
    """Returns dict(depth, normal, albedo, shading, intensity, residual, hit, samples) over (h, w) (normal (h, w, 3)); SH planes only when grid.sh is set."""
    g = grid; vs = g.vs
    d, inv_len = rays(cam)
    eye = cam["eye"]
    n = d.shape[0]
    dl = vs * inv_len
    t0 = np.full(n, float(tmin) if tmin > 0 else 0.0)
    t1 = np.full(n, float(tmax) if tmax > 0 else np.inf)
    for a in range(3):
        B0 = float(int(g.lo[a]) * 8) * vs; B1 = float(int(g.lo[a] + g.dim[a]) * 8) * vs
        nz = d[:, a] != 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            ta = (B0 - eye[a]) / d[:, a]; tb = (B1 - eye[a]) / d[:, a]
        t0 = np.where(nz, np.maximum(t0, np.minimum(ta, tb)), t0)
        t1 = np.where(nz, np.minimum(t1, np.maximum(ta, tb)), np.where((eye[a] < B0) | (eye[a] >= B1), -1.0, t1))

    def pos(idx, t):
        q = np.stack([(eye[a] + t * d[idx, a]) / vs for a in range(3)], -1)
        b = np.floor(q).astype(np.int64)
        return q, b

    t = t0.copy(); pv = np.zeros(n, bool); pt = np.zeros(n); pf = np.zeros(n)
    samples = np.zeros(n, np.int64); hit = np.zeros(n, bool); ta_ = np.zeros(n); fa_ = np.zeros(n); tb_ = np.zeros(n); fb_ = np.zeros(n)
    active = np.ones(n, bool)
    while True:
        active &= (t < t1) & (samples < MAX_SAMPLES)
        idx = np.nonzero(active)[0]
        if idx.size == 0:
            break
        samples[idx] += 1
        q, b = pos(idx, t[idx])
        k = (b >> BRICK_SHIFT) - g.lo[None, :]
        inbox = ((k >= 0) & (k < g.dim[None, :])).all(1)
        o = idx[~inbox]
        pv[o] = False; t[o] += 1e-4 * dl[o]
        idx, q, b, k = idx[inbox], q[inbox], b[inbox], k[inbox]
        bit = g.bits[k[:, 2], k[:, 1], k[:, 0]] if idx.size else np.zeros(0, bool)
        e = idx[~bit]
        if e.size:
            kb = b[~bit] >> BRICK_SHIFT
            te = t1[e].copy()
            for a in range(3):
                da = d[e, a]
                edge = np.where(da > 0.0, (kb[:, a] + 1) * 8, kb[:, a] * 8).astype(np.float64) * vs
                with np.errstate(divide="ignore", invalid="ignore"):
                    te = np.where(da != 0.0, np.minimum(te, (edge - eye[a]) / da), te)
            pv[e] = False; t[e] = np.maximum(t[e], te) + 1e-4 * dl[e]
        idx, q, b = idx[bit], q[bit], b[bit]
        if idx.size == 0:
            continue
        c, v, ok = g.cell(b)
        o = idx[~ok]
        pv[o] = False; t[o] += 0.5 * dl[o]
        idx, q, b, v = idx[ok], q[ok], b[ok], v[ok]
        f = _tri(_weights(q - b), v)
        pos_ = f > 0.0
        o = idx[pos_]
        pv[o] = True; pt[o] = t[o]; pf[o] = f[pos_]; t[o] += np.minimum(np.maximum(f[pos_], 0.25 * vs), vs) * inv_len[o]
        neg = ~pos_
        h = neg & pv[idx] & (pf[idx] > 0.0)
        o = idx[h]
        hit[o] = True; active[o] = False; ta_[o] = pt[o]; fa_[o] = pf[o]; tb_[o] = t[o]; fb_[o] = f[h]
        r = neg & ~h
        o = idx[r]
        pv[o] = True; pt[o] = t[o]; pf[o] = f[r]; t[o] += 0.25 * dl[o]

    def field_at(idx, tt):
        q, b = pos(idx, tt)
        c, v, ok = g.cell(b)
        fr = q - b
        return ok, _tri(_weights(fr), v), c, v, fr

    hi = np.nonzero(hit)[0]
    ta, fa, tb, fb = ta_[hi], fa_[hi], tb_[hi], fb_[hi]
    tc = ta + (tb - ta) * fa / (fa - fb)
    okc, fc, _, _, _ = field_at(hi, tc)
    up = okc & (fc > 0.0); dn = okc & ~(fc > 0.0)
    ta = np.where(up, tc, ta); fa = np.where(up, fc, fa); tb2 = np.where(dn, tc, tb); fb2 = np.where(dn, fc, fb)
    t_hit = np.where(okc, ta + (tb2 - ta) * fa / (fa - fb2), tc)
    okh, _, c, v, fr = field_at(hi, t_hit)
    _, _, cb, vb, frb = field_at(hi, tb_[hi])                    # the hit sample's cell (valid) when t_hit's is not
    c = np.where(okh[:, None], c, cb); v = np.where(okh[:, None], v, vb); fr = np.where(okh[:, None], fr, frb)

    fx, fy, fz = fr[:, 0], fr[:, 1], fr[:, 2]; gx, gy, gz = 1.0 - fx, 1.0 - fy, 1.0 - fz
    nx = (((v[:, 1] - v[:, 0]) * gy * gz + (v[:, 3] - v[:, 2]) * fy * gz) + (v[:, 5] - v[:, 4]) * gy * fz) + (v[:, 7] - v[:, 6]) * fy * fz
    ny = (((v[:, 2] - v[:, 0]) * gx * gz + (v[:, 3] - v[:, 1]) * fx * gz) + (v[:, 6] - v[:, 4]) * gx * fz) + (v[:, 7] - v[:, 5]) * fx * fz
    nz = (((v[:, 4] - v[:, 0]) * gx * gy + (v[:, 5] - v[:, 1]) * fx * gy) + (v[:, 6] - v[:, 2]) * gx * fy) + (v[:, 7] - v[:, 3]) * fx * fy
    nl = np.sqrt((nx * nx + ny * ny) + nz * nz)
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = np.where(nl[:, None] > 0.0, np.stack([nx, ny, nz], -1) / nl[:, None], 0.0)
    w = _weights(fr)
    H, W = cam["h"], cam["w"]
    out = dict(hit=hit.reshape(H, W), samples=samples.reshape(H, W), depth=np.zeros(n), normal=np.zeros((n, 3)))
    out["depth"][hi] = t_hit; out["normal"][hi] = nrm
    if g.alb is not None:
        out["albedo"] = np.zeros(n); out["albedo"][hi] = _tri(w, g.alb[c])
    if g.sh is not None and g.alb is not None:
        Hb = sh_basis(nrm[:, 0], nrm[:, 1], nrm[:, 2])
        shade = np.zeros(hi.size)
        for j in range(9):
            shade = shade + _tri(w, g.sh[c, j]) * Hb[j]
        shade = np.where(nl > 0.0, shade, 0.0)
        out["shading"] = np.zeros(n); out["shading"][hi] = shade
        out["intensity"] = np.zeros(n); out["intensity"][hi] = out["albedo"][hi] * shade
        if lum is not None:
            out["residual"] = np.zeros(n); out["residual"][hi] = out["intensity"][hi].astype(np.float32) - np.asarray(lum, np.float32).ravel()[hi]
    for k in ("depth", "albedo", "shading", "intensity", "residual"):
        if k in out:
            out[k] = out[k].reshape(H, W)
    out["normal"] = out["normal"].reshape(H, W, 3)
    out["dir"] = d.reshape(H, W, 3)
    return out
