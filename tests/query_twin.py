"""numpy statement of i3d_query_points, vectorised over points, in fp64.

Test infrastructure: the device kernel (query_kernels.hip) is compared against this.  It evaluates the same fp64 expressions in the same order as the kernel
(which is compiled without contraction) on the cell of render_twin.Grid, so values agree to rounding and every discrete decision (cell, convergence, step count)
is the same unless an iterate sits on a cell face.
"""
from __future__ import annotations

import numpy as np

import render_twin
from render_twin import Grid, _tri, _weights  # noqa: F401  (Grid re-exported for the tests)

MAX_COORD = 1048576.0          # query_kernels.hpp QUERY_MAX_COORD


def _locate(g: Grid, x):
    """cell of the world points x [M, 3]: (valid, corners [M, 8], values [M, 8], frac [M, 3], q [M, 3]); no lookup for a non-finite or far point"""
    with np.errstate(invalid="ignore", over="ignore"):
        q = x / g.vs
        near = np.isfinite(x).all(1) & (np.abs(q) < MAX_COORD).all(1)
    qs = np.where(near[:, None], q, 0.0)
    b = np.floor(qs).astype(np.int64)
    c, v, ok = g.cell(b)
    return ok & near, c, v, qs - b, q


def _gradient(v, fr):
    fx, fy, fz = fr[:, 0], fr[:, 1], fr[:, 2]; gx, gy, gz = 1.0 - fx, 1.0 - fy, 1.0 - fz
    nx = (((v[:, 1] - v[:, 0]) * gy * gz + (v[:, 3] - v[:, 2]) * fy * gz) + (v[:, 5] - v[:, 4]) * gy * fz) + (v[:, 7] - v[:, 6]) * fy * fz
    ny = (((v[:, 2] - v[:, 0]) * gx * gz + (v[:, 3] - v[:, 1]) * fx * gz) + (v[:, 6] - v[:, 4]) * gx * fz) + (v[:, 7] - v[:, 5]) * fx * fz
    nz = (((v[:, 4] - v[:, 0]) * gx * gy + (v[:, 5] - v[:, 1]) * fx * gy) + (v[:, 6] - v[:, 2]) * gx * fy) + (v[:, 7] - v[:, 3]) * fx * fy
    gr = np.stack([nx, ny, nz], -1)
    return gr, np.sqrt((nx * nx + ny * ny) + nz * nz)


def query(grid: Grid, points, project=True, max_steps=16, tolerance_voxels=1e-6, trace=False):
    """Returns dict(sdf, normal (float32), albedo (float32, when the grid has one), foot, distance, status (uint8), steps (per point), corner_max (max |corner
    value| of the cell at the point), stats).  trace=True adds "trace": a list of (indices, q [m, 3] in voxel units, valid [m]) per evaluation, the start included."""
    g = grid; vs = g.vs
    p0 = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    n = p0.shape[0]
    tol = float(tolerance_voxels) * vs
    ok, c, v, fr, q = _locate(g, p0)
    f = np.where(ok, _tri(_weights(fr), v), 0.0)
    gr, nl = _gradient(v, fr)
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = np.where((ok & (nl > 0.0))[:, None], gr / nl[:, None], 0.0).astype(np.float32)
    out = dict(sdf=f.copy(), normal=nrm, status=ok.astype(np.uint8), corner_max=np.where(ok, np.abs(v).max(1), 0.0))
    if g.alb is not None:
        out["albedo"] = np.where(ok, _tri(_weights(fr), g.alb[c]), 0.0).astype(np.float32)
    foot = np.zeros((n, 3)); dist = np.zeros(n); steps = np.zeros(n, np.int64)
    tr = [(np.arange(n), q.copy(), ok.copy())]
    if project:
        idx = np.nonzero(ok)[0]
        x = p0[idx].copy(); fc = f[idx].copy(); gc = gr[idx].copy(); nc = nl[idx].copy(); it = 0
        while idx.size:
            conv = np.abs(fc) <= tol
            k = idx[conv]
            d = x[conv] - p0[k]
            ln = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            dist[k] = np.where(f[k] > 0.0, ln, np.where(f[k] < 0.0, -ln, 0.0)); foot[k] = x[conv]; out["status"][k] |= 2
            go = ~conv & (nc > 0.0) if it < max_steps else np.zeros(idx.size, bool)
            idx, x, fc, gc, nc = idx[go], x[go], fc[go], gc[go], nc[go]
            if not idx.size:
                break
            s = np.fmin(np.fmax(fc * vs / nc, -vs), vs)
            x = np.stack([x[:, a] - s * (gc[:, a] / nc) for a in range(3)], -1)
            it += 1; steps[idx] = it
            okx, _, vx, frx, qx = _locate(g, x)
            tr.append((idx.copy(), qx.copy(), okx.copy()))
            fc = _tri(_weights(frx), vx)
            gc, nc = _gradient(vx, frx)
            idx, x, fc, gc, nc = idx[okx], x[okx], fc[okx], gc[okx], nc[okx]
    out.update(foot=foot, distance=dist, steps=steps)
    b0 = (out["status"] & 1) != 0; b1 = (out["status"] & 2) != 0
    a0, a1 = np.abs(f[b0]), np.abs(dist[b1])
    out["stats"] = dict(valid=int(b0.sum()), projected=int(b1.sum()), sum_abs_sdf=float(a0.sum()), sum_sq_sdf=float((a0 * a0).sum()),
                        max_abs_sdf=float(a0.max()) if a0.size else 0.0, sum_abs_distance=float(a1.sum()), sum_sq_distance=float((a1 * a1).sum()),
                        max_abs_distance=float(a1.max()) if a1.size else 0.0, steps=int(steps.sum()))
    if trace:
        out["trace"] = tr
    return out


def face_margin(trace):
    """per point: the smallest distance (voxels) of any of its iterates (non-finite / far ones skipped) to a cell face"""
    n = trace[0][0].size
    m = np.full(n, 0.5)
    for idx, q, _ in trace:
        with np.errstate(invalid="ignore"):
            fin = np.isfinite(q).all(1) & (np.abs(q) < MAX_COORD).all(1)
        qq = np.where(fin[:, None], q, 0.5)
        fr = qq - np.floor(qq)
        m[idx] = np.minimum(m[idx], np.minimum(fr, 1.0 - fr).min(1))
    return m


def all_valid(trace):
    """per point: every evaluated iterate lies in a valid cell"""
    n = trace[0][0].size
    a = np.ones(n, bool)
    for idx, _, ok in trace:
        a[idx] &= ok
    return a
