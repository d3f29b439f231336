"""The grids, the seeded point sets and the recorded bars of the point-set registration tests (test_register_cpu.py asserts their input conditions and measures
the bars, test_gpu_register.py compares the device on them).

The grids are the bumpy-sphere shells of query_cases at radius 12 voxels with a bump amplitude (BUMP_VOX) at which the twin's min_pivot_ratio is >= 1e-3, so
that all six degrees of freedom are pinned; the three placements are those of query_cases (plain, shifted by SHIFT, straddling the origin).

A point set is CHECKED: its points are feet of the twin's projection (query_twin.query, project=True) of band points, so they lie on the model's zero set and
the true pose is known; they are moved into a frame of their own by the inverse of TRUE pose; then every point for which, at any sums pass of the twin's run from
any of the three starts, the placed point lies within FACE_MARGIN voxel of a cell face or its |r| within 1e-9 * vs of the gate is replaced by a spare foot, until
none is left.  A last-bit difference of a position can then change neither a cell nor the inlier set.
"""
import functools
import math

import numpy as np

import query_cases as Q
import query_twin
import register_twin as RT
import render_twin
from intrinsic3d_amd import synthetic

VS = Q.VS
FACE_MARGIN = Q.FACE_MARGIN
GATE_MARGIN = 1e-9            # x vs
BUMP_VOX = 12.0               # bump amplitude of the shell (query_cases' default 0.5 gives min_pivot_ratio ~ 2e-5; the ratio is in metre units, ~ lever^2)
N_FULL = 3000
SIZES = (1, 63, 65, 257, N_FULL)
ROW_CAP_P2 = 8                # slab rows allowed through i3d_debug_register_row_cap so that N_FULL points walk two per lane (12 workgroups of 256 > 8)
START_ROT_DEG, START_TRANS_VOX = 1.0, 1.5
STOP_MARGIN = 1e-3            # no step of a twin run has |omega| or |upsilon| within this relative distance of the stop rule

# Recorded by test_register_cpu.py.  Twin against the truth over the 18 runs (3 grids x 2 fields x 3 starts): rotation <= 1.3e-9 rad,
# translation <= 2.1e-8 voxel; the device's bars are twice that, rounded up.
TRUTH_BAR_RAD, TRUTH_BAR_VOX = 3e-9, 5e-8
# the depth-frame case (32 x 24 view, points back-projected from the fp32 depth plane of the render twin): the twin returns to the render pose within
# 1.07e-5 rad / 3.49e-4 voxel (the fp32 depth and the ray cast's own tolerance, not the registration, set this); the device's bars are twice that, rounded up
VIEW_BAR_RAD, VIEW_BAR_VOX = 3e-5, 7e-4


@functools.lru_cache(maxsize=None)
def grid(name):
    if name == "plain":
        return Q.sphere_grid(bump_amp_vox=BUMP_VOX)
    if name == "shifted":
        return Q.sphere_grid(bump_amp_vox=BUMP_VOX, shift=Q.SHIFT)
    g = grid("plain")
    return Q.sphere_grid(bump_amp_vox=BUMP_VOX, shift=-np.round(g["centre_vox"]).astype(np.int64) - np.array([0, 0, g["radius_vox"]]))


GRID_NAMES = ("plain", "shifted", "negative")


def true_pose(g):
    """the points' frame: the world turned by a fixed rotation about a point near the sphere's centre, which becomes its origin"""
    R = synthetic.aa_to_rotmat(np.array([0.2, -0.3, 0.25]))
    t = g["centre_vox"] * VS + np.array([0.3, -0.2, 0.1]) * VS
    return np.concatenate([synthetic.rotmat_to_aa(R), t])


def start_pose(g, k):
    """start k (0..2) of grid g: the true pose turned by START_ROT_DEG about the sphere's centre and moved by START_TRANS_VOX voxels, seeded"""
    rng = np.random.default_rng(100 + k)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    dt = rng.normal(size=3); dt *= START_TRANS_VOX * VS / np.linalg.norm(dt)
    Rt, tt = RT.pose_to_rt(true_pose(g))
    Rd = synthetic.aa_to_rotmat(ax * math.radians(START_ROT_DEG))
    cw = g["centre_vox"] * VS
    return RT.rt_to_pose(Rd @ Rt, Rd @ (tt - cw) + cw + dt)


def to_frame(g, world):
    Rt, tt = RT.pose_to_rt(true_pose(g))
    return (np.asarray(world, np.float64) - tt) @ Rt          # R^T (x - t)


def surface_feet(g, tw_grid, n, seed):
    """n feet of the twin's projection of points within 2 voxels of the shell (outside the +x cap), every walk inside valid cells and off the cell faces"""
    rng = np.random.default_rng(seed)
    out = np.zeros((0, 3))
    scene, off = g["scene"], g["offset"]
    while out.shape[0] < n:
        d = rng.normal(size=(8 * n, 3)); d /= np.sqrt((d * d).sum(1, keepdims=True))
        d = d[d[:, 0] < np.cos(np.radians(35.0))]
        r = g["radius_vox"] + rng.uniform(-BUMP_VOX - 2.0, BUMP_VOX + 2.0, d.shape[0])
        cand = (g["centre_vox"] + d * r[:, None]) * VS
        cand = cand[np.abs(scene.sdf(cand - off)) < 2.0 * VS]
        tw = query_twin.query(tw_grid, cand, trace=True)
        ok = (tw["status"] == 3) & query_twin.all_valid(tw["trace"]) & (query_twin.face_margin(tw["trace"]) >= FACE_MARGIN)
        out = np.concatenate([out, tw["foot"][ok]])
    return out[:n]


def run_margins(grid_tw, pts, st, max_distance):
    """per point over the passes of a traced twin run: (smallest distance of a placed point to a cell face, voxels; smallest | |r| - gate | / vs over valid passes)"""
    face = np.full(pts.shape[0], 0.5); gate = np.full(pts.shape[0], np.inf)
    for a in st["trace"]:
        with np.errstate(invalid="ignore"):
            fin = np.isfinite(a["q"]).all(1) & (np.abs(a["q"]) < query_twin.MAX_COORD).all(1)
        q = np.where(fin[:, None], a["q"], 0.5)
        fr = q - np.floor(q)
        face = np.minimum(face, np.minimum(fr, 1.0 - fr).min(1))
        gate = np.where(a["valid_mask"], np.minimum(gate, np.abs(np.abs(a["r"]) - max_distance) / grid_tw.vs), gate)
    return face, gate


@functools.lru_cache(maxsize=None)
def checked_set(name, refined):
    """(g, points [N_FULL, 3] in their own frame, [(start pose, twin pose, twin stats with trace)] for the three starts)"""
    g = grid(name)
    tw_grid = Q.twin_grid(g, refined)
    feet = surface_feet(g, tw_grid, N_FULL + 600, 40 + GRID_NAMES.index(name) * 2 + int(refined))
    pts = to_frame(g, feet)
    use, spare = pts[:N_FULL].copy(), list(pts[N_FULL:])
    md = RT.default_desc()["max_distance"]
    for _ in range(50):
        runs, bad = [], np.zeros(N_FULL, bool)
        for k in range(3):
            s = start_pose(g, k)
            pose, st = RT.register(tw_grid, use, s, trace=True)
            face, gate = run_margins(tw_grid, use, st, md)
            bad |= (face < FACE_MARGIN) | (gate < GATE_MARGIN)
            runs.append((s, pose, st))
        if not bad.any():
            return g, use, runs
        for i in np.nonzero(bad)[0]:
            use[i] = spare.pop()
    raise AssertionError("the redraw did not settle")


def twin_order_bar(name, refined, k):
    """the device-against-twin bar of start k: 100 x the pose difference between the twin with numpy's sums and with sequential sums, floor 1e-12 (rad, voxel)"""
    g, pts, runs = checked_set(name, refined)
    seq, st = RT.register(Q.twin_grid(g, refined), pts, runs[k][0], order="sequential")
    assert st["status"] == runs[k][2]["status"] and st["iterations"] == runs[k][2]["iterations"]
    ang, tr = RT.pose_diff(seq, runs[k][1], VS)
    return max(100.0 * ang, 1e-12), max(100.0 * tr, 1e-12), (ang, tr)


def empty_points(g, n, seed):
    """points (own frame) that the starts place deep inside the sphere: nothing stored there"""
    rng = np.random.default_rng(seed)
    return to_frame(g, (g["centre_vox"] + rng.uniform(-3, 3, (n, 3))) * VS)


SPECIAL = np.array([[np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, -np.inf], [np.nan, np.nan, np.nan], [1e30, 0.1, 0.1], [0.1, -1e30, 0.1], [1e300, 1e300, 1e300],
                    [1048576.0 * VS * 3.0, 0.0, 0.0], [0.0, -1048576.0 * VS * 3.0, 0.0]])


# ---- the depth-frame case -------------------------------------------------------------------------------------------------------------------------------
def view_case(g, depth):
    """camera-frame points of the hits of a depth plane of query_cases.view_camera (depth * (x, y, 1), render_twin.rays with the identity rotation), the true
    camera -> world pose and a perturbed start"""
    cam = Q.view_camera(g)
    ident = dict(R=np.eye(3), eye=np.zeros(3), intr=cam["intr"], dist=cam["dist"], w=cam["width"], h=cam["height"])
    d, _ = render_twin.rays(ident)
    z = np.asarray(depth, np.float32).reshape(-1).astype(np.float64)
    pts = (d * z[:, None])[z > 0]
    tc = render_twin.camera_from_pose(cam["pose"], cam["intr"], cam["dist"], cam["width"], cam["height"])
    truth = RT.rt_to_pose(tc["R"].T.copy(), tc["eye"])
    rng = np.random.default_rng(7)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    dt = rng.normal(size=3); dt *= 1.0 * VS / np.linalg.norm(dt)
    Rd = synthetic.aa_to_rotmat(ax * math.radians(0.5))
    cw = g["centre_vox"] * VS
    start = RT.rt_to_pose(Rd @ tc["R"].T, Rd @ (tc["eye"] - cw) + cw + dt)
    return pts, truth, start
