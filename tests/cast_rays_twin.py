"""numpy statement of i3d_cast_rays / i3d_fusion_cast_rays, vectorised over rays, in fp64.

Test infrastructure: the device kernel (cast_rays_kernels.hip) is compared against this.  It is the march of render_twin.render with
a per-ray origin, direction and range in place of one camera: the same fp64 expressions in the same order as the kernel, which is compiled without contraction.
Fed the rays of a camera and its eye it must equal render_twin.render exactly (tests/test_cast_rays_cpu.py).
"""
from __future__ import annotations

import numpy as np

from render_twin import Grid, _tri, _weights, camera_from_pose, rays  # noqa: F401

MAX_SAMPLES = 1 << 14          # render_kernels.hpp RENDER_MAX_SAMPLES
BRICK_SHIFT = 3                # 8^3-voxel bricks
MAX_COORD = 1048576.0          # |o / vs| >= 2^20: invalid (query_kernels.hpp QUERY_MAX_COORD)
VALID, HIT, BUDGET = 1, 2, 4   # the status bits


def _sh_basis(nx, ny, nz):
    """the SH basis in the kernel's operation order (hit_attributes, ray_march_device.hpp)"""
    return [np.ones_like(nx), ny, nz, nx, nx * ny, ny * nz, -nx * nx - ny * ny + 2.0 * nz * nz, nx * nz, nx * nx - ny * ny]


def ray_ranges(origins, dirs, vs, t_min=None, t_max=None):
    """valid [n], a [n], b [n]: the rule of DESIGN.md 34.1 for invalid rays and open ranges"""
    o = np.asarray(origins, np.float64).reshape(-1, 3); d = np.asarray(dirs, np.float64).reshape(-1, 3)
    n = o.shape[0]
    lo = np.zeros(n) if t_min is None else np.asarray(t_min, np.float64).reshape(n)
    hi = np.zeros(n) if t_max is None else np.asarray(t_max, np.float64).reshape(n)
    with np.errstate(all="ignore"):
        l2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (np.abs(o / vs) < MAX_COORD).all(1)
        valid &= (l2 > 0.0) & np.isfinite(l2) & ~np.isnan(lo) & ~np.isnan(hi) & ~(lo == np.inf)
        a = np.where(lo > 0.0, lo, 0.0); b = np.where(hi > 0.0, hi, np.inf)
    return valid, a, b


def cast(grid: Grid, origins, dirs, t_min=None, t_max=None):
    """Returns dict(valid, hit, samples, status, t, position, normal, albedo, shading, intensity) over the n rays; albedo only when grid.alb is set, the SH outputs
    only when grid.sh is set too."""
    g = grid; vs = g.vs
    o_all = np.asarray(origins, np.float64).reshape(-1, 3); d_all = np.asarray(dirs, np.float64).reshape(-1, 3)
    n = o_all.shape[0]
    valid, a_, b_ = ray_ranges(o_all, d_all, vs, t_min, t_max)
    eye = np.where(valid[:, None], o_all, 0.0)                         # an invalid ray is never marched: a placeholder keeps the arithmetic quiet
    d = np.where(valid[:, None], d_all, np.array([0.0, 0.0, 1.0]))
    inv_len = 1.0 / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    dl = vs * inv_len
    t0 = a_.copy(); t1 = b_.copy()
    for a in range(3):
        B0 = float(int(g.lo[a]) * 8) * vs; B1 = float(int(g.lo[a] + g.dim[a]) * 8) * vs
        nz = d[:, a] != 0.0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            ta = (B0 - eye[:, a]) / d[:, a]; tb = (B1 - eye[:, a]) / d[:, a]
        t0 = np.where(nz, np.maximum(t0, np.minimum(ta, tb)), t0)
        t1 = np.where(nz, np.minimum(t1, np.maximum(ta, tb)), np.where((eye[:, a] < B0) | (eye[:, a] >= B1), -1.0, t1))

    def pos(idx, t):
        q = np.stack([(eye[idx, a] + t * d[idx, a]) / vs for a in range(3)], -1)
        b = np.floor(q).astype(np.int64)
        return q, b

    t = t0.copy(); pv = np.zeros(n, bool); pt = np.zeros(n); pf = np.zeros(n)
    samples = np.zeros(n, np.int64); hit = np.zeros(n, bool); ta_ = np.zeros(n); fa_ = np.zeros(n); tb_ = np.zeros(n); fb_ = np.zeros(n)
    active = valid.copy()
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
                with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                    te = np.where(da != 0.0, np.minimum(te, (edge - eye[e, a]) / da), te)
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
    status = np.where(valid, VALID | np.where(hit, HIT, 0) | np.where(~hit & (samples >= MAX_SAMPLES), BUDGET, 0), 0).astype(np.uint8)
    out = dict(valid=valid, hit=hit, samples=samples, status=status, t=np.zeros(n), position=np.zeros((n, 3)), normal=np.zeros((n, 3)))
    out["t"][hi] = t_hit; out["normal"][hi] = nrm
    out["position"][hi] = eye[hi] + t_hit[:, None] * d[hi]
    if g.alb is not None:
        out["albedo"] = np.zeros(n); out["albedo"][hi] = _tri(w, g.alb[c])
    if g.sh is not None and g.alb is not None:
        Hb = _sh_basis(nrm[:, 0], nrm[:, 1], nrm[:, 2])
        shade = np.zeros(hi.size)
        for j in range(9):
            shade = shade + _tri(w, g.sh[c, j]) * Hb[j]
        shade = np.where(nl > 0.0, shade, 0.0)
        out["shading"] = np.zeros(n); out["shading"][hi] = shade
        out["intensity"] = np.zeros(n); out["intensity"][hi] = out["albedo"][hi] * shade
    return out
