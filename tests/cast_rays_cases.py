"""The scene and the ray sets that tests/test_cast_rays_cpu.py and tests/test_gpu_cast_rays.py share (test infrastructure, no tests in here).

The scene is the one of tests/test_gpu_render.py: helpers.small_scene(radius_vox=12, width=96, height=72), the refined field and the albedo perturbed.  The
CPU test builds the twin's grid from these arrays; the GPU tests build it from what the context exports, which is the same values.
"""
from __future__ import annotations

import numpy as np

import helpers
import render_twin
from intrinsic3d_amd import synthetic

DIST = helpers.TRACK_DIST
SHIFT = (-100000, -99987, -100021)


def scene(shift=None, levels=1, seed=5):
    sc = dict(helpers.small_scene(seed=seed, radius_vox=12, K=3, width=96, height=72, levels=levels))
    vs = float(sc["voxel_size"])
    sc["albedo_true"] = sc["scene"].albedo(sc["keys"].astype(np.float64) * vs)
    sc["shift_m"] = np.zeros(3)
    if shift is not None:                            # the same scene in the negative octant, far from the origin (world shifted by t: tr' = tr - R t)
        shift = np.asarray(shift, np.int64)
        sc["keys"] = (sc["keys"] + shift[None, :]).astype(np.int32)
        t = shift.astype(np.float64) * vs
        poses = np.array(sc["poses"], np.float64)
        for f in range(len(poses)):
            poses[f, 3:] = poses[f, 3:] - synthetic.aa_to_rotmat(poses[f, :3]) @ t
        sc["poses"] = poses
        sc["shift_m"] = t
    return sc


def perturbed(sc, seed=11):
    rng = np.random.default_rng(seed)
    vs = float(sc["voxel_size"]); n = sc["keys"].shape[0]
    return sc["sdf"].astype(np.float64) + rng.normal(0.0, 0.05 * vs, n), sc["albedo_true"] + rng.normal(0.0, 0.01, n)


def cpu_grid(sc, refined=True):
    """the twin's grid from the scene's arrays: what a context holds after set_grid(perturbed) and set_voxel_sh(SH_TRUE)"""
    sdf_r, alb = perturbed(sc)
    n = sc["keys"].shape[0]
    return render_twin.Grid(sc["keys"], sdf_r if refined else sc["sdf"], sc["weight"], sc["voxel_size"], albedo=alb, sh=np.tile(synthetic.SH_TRUE, (n, 1)))


def front_camera(sc):
    """The free camera of the bit-for-bit tests: zero rotation, zero distortion, translated so that the object fills the view.  With a zero rotation vector the
    library's pose takes its small-angle branch and gives the identity exactly, so eye = -t and d = ((u - cx) / fx, (v - cy) / fy, 1) are what numpy computes."""
    w, h = 96, 72
    f = 150.0
    centre = sc["center"] + sc["shift_m"]
    eye = centre - np.array([0.0, 0.0, 0.16])                         # the sphere of radius 0.048 at z = 0.16: 0.3 x 150 = 45 of 72 pixels
    cam = dict(width=w, height=h, intr=np.array([f, f, (w - 1) * 0.5, (h - 1) * 0.5]), dist=np.zeros(5), pose=np.concatenate([np.zeros(3), -eye]))
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    d = np.stack([((u - cam["intr"][2]) / f).ravel(), ((v - cam["intr"][3]) / f).ravel(), np.ones(w * h)], -1)
    o = np.broadcast_to(-cam["pose"][3:], d.shape).copy()
    return cam, o, d


def general_rays(sc, grid, seed=21, per_kind=900):
    """The general ray set of DESIGN.md 34's tests -> (origins, directions, t_min, t_max), every ray valid.
    Origins: on a sphere of three object radii, uniform in the bitmap's box, inside the surface (between 0.2 and 0.97 radii from the centre).  Directions aim at
    jittered points of the box, with lengths in [0.5, 3].  Ranges by thirds: open; t_max at 0.8 of the way to the sphere of the object's radius (short of the
    surface); t_min three voxels past that crossing (the ray starts inside the surface); a ray that does not meet that sphere from outside has 0.8 of / half the
    way to its target instead.  Then axis-parallel rays with exact zeros in d, inside and outside the
    box's slab on the zero axes."""
    rng = np.random.default_rng(seed)
    vs = grid.vs
    c = sc["center"] + sc["shift_m"]; R = sc["scene"].R
    B0 = grid.lo.astype(np.float64) * 8 * vs; B1 = (grid.lo + grid.dim).astype(np.float64) * 8 * vs

    def unit(m):
        x = rng.normal(size=(m, 3))
        return x / np.linalg.norm(x, axis=1, keepdims=True)

    o = np.concatenate([c + 3.0 * R * unit(per_kind), B0 + (B1 - B0) * rng.random((per_kind, 3)), c + R * rng.uniform(0.2, 0.97, (per_kind, 1)) * unit(per_kind)])
    n = o.shape[0]
    target = B0 + (B1 - B0) * rng.random((n, 3))
    d = target - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.5, 3.0, (n, 1))
    # the first crossing of the sphere |x - c| = R from outside, in units of d (inf: none)
    oc = o - c; A = (d * d).sum(1); Bq = (oc * d).sum(1); Cq = (oc * oc).sum(1) - R * R
    disc = Bq * Bq - A * Cq
    with np.errstate(invalid="ignore"):
        ts = np.where((disc > 0) & (Cq > 0), (-Bq - np.sqrt(np.maximum(disc, 0.0))) / A, np.inf)
    ts = np.where(ts > 0, ts, np.inf)
    kind = rng.permutation(n) % 3
    t_min = np.zeros(n); t_max = np.zeros(n)
    meets = np.isfinite(ts)
    to_target = np.linalg.norm(target - o, axis=1) / np.sqrt(A)           # a ray that never meets the sphere from outside: its range is cut at its target instead
    short = kind == 1; past = kind == 2
    t_max[short] = 0.8 * np.where(meets, ts, to_target)[short]
    t_min[past] = np.where(meets, ts + 3.0 * vs / np.sqrt(A), 0.5 * to_target)[past]
    # axis-parallel rays: one or two exact zeros in d; origins inside the slab of the zero axes (through the object) and outside it (beside the box)
    ao, ad = [], []
    for axis in range(3):
        for sign in (1.0, -1.0):
            for m in range(40):
                p = c + R * 1.2 * (rng.random(3) - 0.5)
                p[axis] = c[axis] - sign * 2.5 * R
                if m % 4 == 3:
                    p[(axis + 1) % 3] = B1[(axis + 1) % 3] + (0.0 if m % 8 == 3 else 2.0 * vs)      # on the box's upper face (outside: the slab is half open) / beyond it
                if m % 4 == 2:
                    p[(axis + 2) % 3] = B0[(axis + 2) % 3] - 1.5 * vs
                e = np.zeros(3); e[axis] = sign * rng.uniform(0.5, 3.0)
                if m % 5 == 0:
                    e[(axis + 1) % 3] = 0.3 * e[axis]                                                 # one zero only
                ao.append(p); ad.append(e)
    o = np.concatenate([o, np.array(ao)]); d = np.concatenate([d, np.array(ad)])
    t_min = np.concatenate([t_min, np.zeros(len(ao))]); t_max = np.concatenate([t_max, np.zeros(len(ao))])
    return o, d, t_min, t_max


def invalid_rays(vs):
    """(origin, direction, t_min, t_max) of one ray per way of being invalid, around the valid ray ((0, 0, 0), (0, 0, 1), 0, 0)"""
    nan, inf = np.nan, np.inf
    big = 1048576.0 * vs
    rows = [((nan, 0, 0), (0, 0, 1), 0, 0), ((0, inf, 0), (0, 0, 1), 0, 0), ((0, 0, -inf), (0, 0, 1), 0, 0), ((0, 0, 0), (nan, 0, 1), 0, 0),
            ((0, 0, 0), (0, -inf, 1), 0, 0), ((0, 0, 0), (0, 0, inf), 0, 0), ((0, 0, 0), (0, 0, 1), nan, 0), ((0, 0, 0), (0, 0, 1), 0, nan),
            ((0, 0, 0), (0, 0, 1), inf, 0), ((0, 0, 0), (0, 0, 0), 0, 0), ((0, 0, 0), (1e200, 0, 0), 0, 0), ((0, 0, 0), (1e-200, 0, 0), 0, 0),
            ((big, 0, 0), (0, 0, 1), 0, 0), ((0, -big, 0), (0, 0, 1), 0, 0), ((0, 0, 2 * big), (0, 0, 1), 0, 0)]
    o = np.array([r[0] for r in rows], np.float64); d = np.array([r[1] for r in rows], np.float64)
    return o, d, np.array([r[2] for r in rows], np.float64), np.array([r[3] for r in rows], np.float64)
