"""numpy statement of i3d_fusion_merge: one volume fused into another under x_dst = R x_src + t.

Test infrastructure: the device kernels (merge_sample, k_merge_alloc, k_merge in fusion_kernels.hip) are compared against this bit for bit.  A volume is a dict(keys
int [n, 3], sdf f32 [n], weight f32 [n], color u8 [n, 3], first_frame i64 [n]) over ALL its stored voxels, those of weight 0 included (Fusion.debug_voxels over a
box that holds them).  The sample of a lattice point is evaluated in float64 on query_twin's cell in the order of tri_weights / tri_sum; the update is
fusion_deintegrate_twin.integrate, float32 in sample_add's order.  R and t / vs are the call's own (its stats), t the caller's pose."""
import numpy as np

import fusion_deintegrate_twin as DT
import query_twin as QT
from render_twin import _tri, _weights

F = np.float32
RANGE = 1 << 20                                     # packed keys hold coordinates strictly inside +- 2^20
OFF = np.array([[i & 1, (i >> 1) & 1, i >> 2] for i in range(8)], np.int64)


def volume(keys=None, sdf=None, weight=None, color=None, first_frame=None):
    n = 0 if keys is None else len(keys)
    return dict(keys=np.zeros((0, 3), np.int64) if keys is None else np.asarray(keys, np.int64).reshape(-1, 3),
                sdf=np.zeros(n, F) if sdf is None else np.asarray(sdf, F), weight=np.zeros(n, F) if weight is None else np.asarray(weight, F),
                color=np.zeros((n, 3), np.uint8) if color is None else np.asarray(color, np.uint8).reshape(-1, 3),
                first_frame=np.zeros(n, np.int64) if first_frame is None else np.asarray(first_frame, np.int64))


def in_range(k):
    return ((k > -RANGE) & (k < RANGE)).all(-1)


def aligned_of(pose6, vs):
    """the host's decision: (aligned, m).  Aligned: no pose, or rotation entries +-0 and every t[a] / (double)vs a whole number of magnitude < 2^20"""
    if pose6 is None:
        return True, np.zeros(3, np.int64)
    p = np.asarray(pose6, np.float64).reshape(6)
    tv = p[3:] / float(F(vs))
    ok = bool((p[:3] == 0.0).all() and (np.trunc(tv) == tv).all() and (np.abs(tv) < RANGE).all())
    return ok, (tv.astype(np.int64) if ok else None)


def sample_aligned(src, m, k):
    """the src voxel k - m as it is, where it is stored with weight != 0"""
    k = np.asarray(k, np.int64).reshape(-1, 3)
    at = DT.lookup(src, np.where(in_range(k - m)[:, None], k - m, 0))
    on = at["found"] & in_range(k - m) & (at["weight"] != 0)
    z = lambda a: np.where(on if a.ndim == 1 else on[:, None], a, a.dtype.type(0))  # noqa: E731
    return dict(on=on, sample=z(at["sdf"]), wu=z(at["weight"]), has_color=on.copy(), rgb=z(at["color"]))


def sample_general(src, vs, R, t, k):
    """p = R^T (k vs - t); where the cell of i3d_fusion_query_points at p in src is valid: trilinear sdf, weight and colour (rounded to nearest), all in float64"""
    k = np.asarray(k, np.int64).reshape(-1, 3); n = k.shape[0]
    out = dict(on=np.zeros(n, bool), sample=np.zeros(n, F), wu=np.zeros(n, F), has_color=np.zeros(n, bool), rgb=np.zeros((n, 3), np.uint8))
    if n == 0 or len(src["keys"]) == 0:
        return out
    R = np.asarray(R, np.float64).reshape(3, 3); t = np.asarray(t, np.float64).reshape(3)
    vsd = float(F(vs))
    d = k.astype(np.float64) * vsd - t
    p = np.stack([(R[0, a] * d[:, 0] + R[1, a] * d[:, 1]) + R[2, a] * d[:, 2] for a in range(3)], -1)
    g = QT.Grid(src["keys"], src["sdf"].astype(np.float64), src["weight"], vsd)
    ok, c, v, fr, _ = QT._locate(g, p)
    w = _weights(fr)
    out["on"] = ok; out["has_color"] = ok.copy()
    out["sample"] = np.where(ok, _tri(w, v), 0.0).astype(F)
    out["wu"] = np.where(ok, _tri(w, src["weight"][c].astype(np.float64)), 0.0).astype(F)
    for ch in range(3):
        out["rgb"][:, ch] = np.where(ok, _tri(w, src["color"][c][:, :, ch].astype(np.float64)) + 0.5, 0.0).astype(np.uint8)
    return out


def candidates(src, R=None, tv=None, m=None):
    """k_merge_alloc's candidate set: per src voxel of weight != 0 the point k + m (aligned, m given), else the 8 points floor(a) + {0,1}^3 around a = R k + t / vs"""
    k = src["keys"][src["weight"] != 0].astype(np.int64)
    if m is not None:
        c = k + np.asarray(m, np.int64)
    else:
        R = np.asarray(R, np.float64).reshape(3, 3); tv = np.asarray(tv, np.float64).reshape(3)
        kd = k.astype(np.float64)
        a = np.stack([((R[a, 0] * kd[:, 0] + R[a, 1] * kd[:, 1]) + R[a, 2] * kd[:, 2]) + tv[a] for a in range(3)], -1)
        a = a[(np.abs(a) < RANGE).all(1)]
        c = (np.floor(a).astype(np.int64)[:, None, :] + OFF[None, :, :]).reshape(-1, 3)
    c = c[in_range(c)]
    _, idx = np.unique(DT.pack(c), return_index=True)                 # ascending packed key
    return c[idx]


def clip_ok(k, vs, clip):
    """k_alloc_centres' clip test: float32 world coordinates of the lattice point against the box"""
    if clip is None or not np.any(np.asarray(clip, F)):
        return np.ones(len(k), bool)
    c = np.asarray(clip, F); w = k.astype(F) * F(vs)
    return ~((w[:, 0] < c[0]) | (w[:, 0] > c[1]) | (w[:, 1] < c[2]) | (w[:, 1] > c[3]) | (w[:, 2] < c[4]) | (w[:, 2] > c[5]))


def merge(dst, src, vs, ordinal, R=None, t=None, tv=None, m=None, clip=None):
    """dst (+) T(src): (volume, stats).  Aligned when m is given.  The inserted voxels follow dst's in ascending order of packed key, which is their rank order."""
    sample = (lambda k: sample_aligned(src, np.asarray(m, np.int64), k)) if m is not None else (lambda k: sample_general(src, vs, R, t, k))
    cand = candidates(src, R, tv, m)
    new = cand[~DT.lookup(dst, cand)["found"] & clip_ok(cand, vs, clip)] if len(cand) else cand
    new = new[sample(new)["on"]] if len(new) else new
    keys = np.concatenate([dst["keys"].astype(np.int64), new]); n0, n1 = len(dst["keys"]), len(new)
    before = dict(sdf=np.concatenate([dst["sdf"], np.zeros(n1, F)]), weight=np.concatenate([dst["weight"], np.zeros(n1, F)]),
                  color=np.concatenate([dst["color"], np.zeros((n1, 3), np.uint8)]))
    smp = sample(keys)
    out = DT.integrate(before, smp)
    out.update(keys=keys, first_frame=np.concatenate([dst["first_frame"], np.full(n1, ordinal, np.int64)]))
    assert smp["on"][n0:].all()
    return out, dict(ordinal=int(ordinal), source_voxels=int((src["weight"] != 0).sum()), sampled=int(smp["on"].sum()), allocated=int(n1), aligned=int(m is not None))
