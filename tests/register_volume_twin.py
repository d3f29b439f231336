"""numpy statement of i3d_fusion_register_volume, vectorised over the samples, in fp64.

Test infrastructure: the device kernels (register_volume_kernels.hip, the step of track_kernels.hip) are compared against this.  A source volume is a dict in
fusion_merge_twin.volume() form over ALL its stored voxels; the volume registered against is query_twin's Grid.  The selection is exact (keys and float sdf, in
ascending packed key).  The placed points, the cell, the residual r = f(R p + t) - s and the Jacobian use the same fp64 expressions in the same order as the kernel
(compiled without contraction); the 6x6 step is track_twin.solve / apply_step.  Only the order of the sums over the samples differs (numpy's pairwise, or
sequential with order="sequential"), so per-sample terms agree to the bit and every discrete decision (cell, inlier, stop) is the same unless a placed point sits on
a cell face, a residual on the gate or a step on the stop rule.
"""
from __future__ import annotations

import math

import numpy as np

import fusion_deintegrate_twin as DT
import query_twin
import register_twin
import track_twin
from register_twin import pose_diff, pose_to_rt, rt_to_pose  # noqa: F401  (re-exported for the tests)

F = np.float32
MIN_INLIERS = track_twin.MIN_INLIERS
UPPER = track_twin.UPPER


def default_desc(**kw):
    d = dict(iterations=30, stride=1, source_band_voxels=2.0, max_distance=0.05, stop_rotation=1e-6, stop_translation=1e-6)
    d.update(kw)
    return d


def select(src, vs_src, source_band_voxels=2.0, stride=1):
    """items 2 and 3: dict(keys int64 [n, 3], sdf float32 [n], points float64 [n, 3]) in ascending packed key"""
    vs = float(F(vs_src))
    band = float(source_band_voxels) * vs
    k = np.asarray(src["keys"], np.int64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        on = (src["weight"] != 0) & (np.abs(src["sdf"].astype(np.float64)) <= band)
    on &= (np.mod(k, int(stride)) == 0).all(1)                     # numpy's modulus is the floor modulus
    k, s = k[on], np.asarray(src["sdf"], F)[on]
    order = np.argsort(DT.pack(k), kind="stable")
    k, s = k[order], s[order]
    return dict(keys=k, sdf=s, points=k.astype(np.float64) * vs)


def _place(R, t, p):
    return np.stack([((R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1]) + R[a, 2] * p[:, 2]) + t[a] for a in range(3)], -1)


def pivot(grid, sel, pose6):
    """item 4: c = R0 mean(p) + t0 over the samples whose placed position counts"""
    return register_twin.pivot(grid, sel["points"], pose6)


def sums(grid, sel, R, tp, c, max_distance, order="numpy", limit=0):
    """one pass of k_register_volume at the pose (R, t' = t - c) about the pivot c over the first `limit` samples (0: all): dict(sums [29], abs_sums [29]
    (sum |term|), valid, inliers, n, face_margin (voxels: the least distance of a placed point to a cell face), gate_margin (metres: the least | |r| - gate | over
    the valid samples))"""
    m = len(sel["keys"]) if not limit else min(int(limit), len(sel["keys"]))
    p = sel["points"][:m]; s = sel["sdf"][:m].astype(np.float64)
    vs = grid.vs
    xp = _place(R, tp, p)
    x = np.stack([xp[:, a] + c[a] for a in range(3)], -1)
    if len(grid.keys):
        ok, _, v, fr, q = query_twin._locate(grid, x)
    else:
        ok = np.zeros(m, bool); v = np.zeros((m, 8)); fr = np.zeros((m, 3)); q = x / vs
    r = np.where(ok, query_twin._tri(query_twin._weights(fr), v) - s, 0.0)
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
        tot = np.ascontiguousarray(T.T).sum(1)
    fin = np.isfinite(q).all(1)
    f = q[fin] - np.floor(q[fin])
    face = float(np.minimum(f, 1.0 - f).min()) if f.size else 0.5
    gate = float(np.abs(np.abs(r[ok]) - max_distance).min()) if ok.any() else math.inf
    return dict(sums=tot, abs_sums=np.abs(T).sum(0), valid=int(ok.sum()), inliers=int(inl.sum()), n=m, face_margin=face, gate_margin=gate, r=r, valid_mask=ok,
                inlier_mask=inl)


def _rms(s):
    return math.sqrt(s[27] / s[28]) if s[28] > 0 else 0.0


def register(grid, src, vs_src, pose6, desc=None, order="numpy"):
    """i3d_fusion_register_volume of the volume src (fusion_merge_twin.volume form, voxel size vs_src) against grid.  Returns (pose6, stats); stats has the fields
    of i3d_register_volume_stats and "face_margin" / "gate_margin", the least over every pass."""
    d = default_desc() if desc is None else default_desc(**desc)
    pose6 = np.asarray(pose6, np.float64)
    sel = select(src, vs_src, d["source_band_voxels"], d["stride"])
    st = dict(iterations=0, status=2, valid=0, inliers=0, rms_initial=0.0, rms_final=0.0, min_pivot_ratio=0.0, selected=len(sel["keys"]), face_margin=0.5,
              gate_margin=math.inf)
    if st["selected"] == 0:
        return pose6.copy(), st
    R, t = pose_to_rt(pose6)
    c = pivot(grid, sel, pose6)
    tp = np.array([t[a] - c[a] for a in range(3)])
    n_it, status = 0, 1

    def one():
        a = sums(grid, sel, R, tp, c, d["max_distance"], order)
        st["face_margin"] = min(st["face_margin"], a["face_margin"]); st["gate_margin"] = min(st["gate_margin"], a["gate_margin"])
        return a

    for k in range(d["iterations"]):
        a = one()
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
        if nw < d["stop_rotation"] and nu < d["stop_translation"]:
            status = 0
            break
    a = one()
    st.update(iterations=n_it, valid=a["valid"], inliers=a["inliers"], rms_final=_rms(a["sums"]))
    if d["iterations"] == 0:
        st["rms_initial"] = st["rms_final"]
        status = 2 if a["inliers"] < MIN_INLIERS else 1
    st["status"] = status
    out = rt_to_pose(R, np.array([tp[a_] + c[a_] for a_ in range(3)])) if n_it > 0 else pose6.copy()
    return out, st
