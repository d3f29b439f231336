"""The grids and the seeded point sets of the point-query tests (test_query_cpu.py asserts their input condition, test_gpu_query.py compares the device on them).

A projection point set is CHECKED: drawn under a fixed seed, then every point whose twin walk breaks the condition the device comparison relies on is redrawn
from the same generator until none is left, so the set is final:
  - every iterate of a point meant to converge lies in a valid cell;
  - no iterate of any point lies within FACE_MARGIN voxel of a cell face (there a last-bit difference of a position could pick another cell).
"""
import functools

import numpy as np

import query_twin
from intrinsic3d_amd import synthetic

VS = float(np.float32(0.004))          # the voxel size as the library stores it
FACE_MARGIN = 1e-9
SHIFT = np.array([-100000, -99987, -100021], np.int64)
BAND = 3.2


def sphere_grid(radius_vox=12, bump_amp_vox=0.5, seed=3, shift=None, hole=True):
    """dict(keys, sdf (fp64 fused), sdf_refined, albedo, weight, color, scene, centre_vox): the bumpy sphere's shell.  One voxel near the surface has weight 0
    (the 8 cells around it are invalid, each by exactly one corner), and with hole=True the voxels of a cap around +x with |sdf| < 1 voxel are not stored: a walk
    that starts outside that cap leaves the stored band."""
    margin = int(np.ceil(radius_vox + BAND + 4))
    scene = synthetic.Scene(np.full(3, (margin + 2) * VS), radius_vox * VS, bump_amp_vox * VS, 40.0)
    keys, _ = synthetic.shell_voxels(scene, VS, BAND, (0, 0, 0), (2 * margin + 4,) * 3)
    P = keys.astype(np.float64) * VS
    sdf = scene.sdf(P)
    if hole:
        d = P - scene.c
        cap = d[:, 0] / np.sqrt((d * d).sum(1)) > np.cos(np.radians(25.0))
        keep = ~(cap & (np.abs(sdf) < 1.0 * VS))
        keys, P, sdf = keys[keep], P[keep], sdf[keep]
    rng = np.random.default_rng(seed)
    n = keys.shape[0]
    perm = rng.permutation(n)
    keys, P, sdf = keys[perm], P[perm], sdf[perm]
    weight = np.ones(n, np.float32)
    d = P - scene.c
    on_minus_y = np.argmin(np.abs(sdf) + 10.0 * np.abs(d[:, 0]) + 10.0 * np.abs(d[:, 2]) + np.where(d[:, 1] < 0, 0.0, 1.0))
    weight[on_minus_y] = 0.0
    g = dict(keys=keys.astype(np.int32), sdf=sdf, sdf_refined=sdf + rng.normal(0.0, 0.02 * VS, n), albedo=scene.albedo(P) + rng.normal(0.0, 0.01, n),
             weight=weight, color=np.full((n, 3), 128, np.uint8), scene=scene, centre_vox=scene.c / VS, radius_vox=radius_vox, hole_voxel=keys[on_minus_y].astype(np.int64),
             offset=np.zeros(3))
    if shift is not None:
        g["keys"] = (g["keys"].astype(np.int64) + np.asarray(shift, np.int64)).astype(np.int32)
        g["offset"] = np.asarray(shift, np.float64) * VS
        g["centre_vox"] = g["centre_vox"] + np.asarray(shift, np.float64)
        g["hole_voxel"] = g["hole_voxel"] + np.asarray(shift, np.int64)
    return g


def twin_grid(g, refined=True):
    return query_twin.Grid(g["keys"], g["sdf_refined"] if refined else g["sdf"], g["weight"], VS, albedo=g["albedo"])


def _band_points(g, rng, n, spread_vox=2.0, avoid_cap=True):
    """points at the sphere's radius +- spread_vox voxels in random directions (outside the +x cap, whose walks are a case of their own)"""
    out = np.zeros((0, 3))
    while out.shape[0] < n:
        d = rng.normal(size=(2 * n, 3)); d /= np.sqrt((d * d).sum(1, keepdims=True))
        if avoid_cap:
            d = d[d[:, 0] < np.cos(np.radians(35.0))]
        r = g["radius_vox"] + rng.uniform(-spread_vox, spread_vox, d.shape[0])
        out = np.concatenate([out, (g["centre_vox"] + d * r[:, None]) * VS])
    return out[:n]


def checked_points(g, n, seed, refined=True, **desc):
    """the checked projection set of grid g: (points [n, 3], twin result).  Every point is meant to converge."""
    rng = np.random.default_rng(seed)
    grid = twin_grid(g, refined)
    pts = _band_points(g, rng, n)
    for _ in range(50):
        tw = query_twin.query(grid, pts, trace=True, **desc)
        bad = ~query_twin.all_valid(tw["trace"]) | (query_twin.face_margin(tw["trace"]) < FACE_MARGIN) | ((tw["status"] & 2) == 0)
        if not bad.any():
            return pts, tw
        pts[bad] = _band_points(g, rng, int(bad.sum()))
    raise AssertionError("the redraw did not settle")


def cap_points(g, n, seed, refined=True):
    """points outside the surface inside the +x cap whose cell is valid and whose walk steps into the voxels that are not stored (twin status 1), none of their
    iterates within FACE_MARGIN of a face: candidates drawn under the seed, the first n that qualify"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(40 * n, 3)) * 0.12 + np.array([1.0, 0.0, 0.0]); d /= np.sqrt((d * d).sum(1, keepdims=True))
    d = d[d[:, 0] > np.cos(np.radians(15.0))]
    r = g["radius_vox"] + rng.uniform(1.4, 2.4, d.shape[0])
    pts = (g["centre_vox"] + d * r[:, None]) * VS
    tw = query_twin.query(twin_grid(g, refined), pts, trace=True)
    ok = (tw["status"] == 1) & (query_twin.face_margin(tw["trace"]) >= FACE_MARGIN)
    assert ok.sum() >= n, ok.sum()
    return pts[ok][:n]


def value_points(g, seed, n_band=3000):
    """the value-query set: band points, empty space, exact voxel centres, q = -0.5 and q just below an integer (negative coordinates), the cells around the
    voxel of weight 0, non-finite and huge coordinates"""
    rng = np.random.default_rng(seed)
    keys = g["keys"].astype(np.int64)
    pick = keys[rng.choice(keys.shape[0], 300, replace=False)]
    hv = g["hole_voxel"]
    around = np.array([[i, j, k] for i in (-2, -1, 0, 1) for j in (-2, -1, 0, 1) for k in (-2, -1, 0, 1)], np.int64)
    below = pick[:100].astype(np.float64)
    below[:, 0] = np.nextafter(below[:, 0], -np.inf)              # q just below an integer: the cell one lower in x
    special = np.array([[np.nan, 0.1, 0.1], [0.1, np.inf, 0.1], [0.1, 0.1, -np.inf], [1e30, 0.1, 0.1], [0.1, -1e30, 0.1], [1e300, 1e300, 1e300],
                        [1048576.0 * VS * 1.5, 0.0, 0.0], [-0.5 * VS, -0.5 * VS, -0.5 * VS], [-0.5 * VS, 0.3 * VS, 0.2 * VS]])
    return np.concatenate([_band_points(g, rng, n_band, spread_vox=2.5, avoid_cap=False),
                           (g["centre_vox"] + rng.uniform(-6, 6, (200, 3))) * VS,                        # inside the sphere: nothing stored
                           (g["centre_vox"] + rng.uniform(-40, 40, (200, 3))) * VS,
                           pick.astype(np.float64) * VS,                                                  # fraction 0: (k * vs) / vs == k (asserted in test_query_cpu.py)
                           below * VS,
                           (hv[None, :] + around).astype(np.float64) * VS + rng.uniform(0.05, 0.95, (around.shape[0], 3)) * VS,
                           special])


def value_segments(n_band=3000):
    """where the cases of value_points lie in its array"""
    o = n_band + 400
    return dict(band=slice(0, n_band), empty=slice(n_band, o), centres=slice(o, o + 300), below=slice(o + 300, o + 400), around=slice(o + 400, o + 464),
                special=slice(o + 464, o + 473))


@functools.lru_cache(maxsize=None)
def plain():
    return sphere_grid()


@functools.lru_cache(maxsize=None)
def shifted():
    return sphere_grid(shift=SHIFT)


@functools.lru_cache(maxsize=None)
def negative():
    """the sphere moved so that its surface passes through the origin (at its +z pole): negative coordinates, the cell based at (-1, -1, -1) is valid"""
    g = plain()
    return sphere_grid(shift=-np.round(g["centre_vox"]).astype(np.int64) - np.array([0, 0, g["radius_vox"]]))


GRIDS = {"plain": plain, "shifted": shifted, "negative": negative}
# the checked projection sets the device is compared on: (grid, points, seed, refined)
PROJECTION_SETS = [("plain", 2500, 11, True), ("plain", 1000, 12, False), ("shifted", 1000, 13, True), ("negative", 1000, 14, True)]


@functools.lru_cache(maxsize=None)
def projection_set(i):
    name, n, seed, refined = PROJECTION_SETS[i]
    g = GRIDS[name]()
    pts, tw = checked_points(g, n, seed, refined)
    return g, refined, pts, tw


def view_camera(g, width=32, height=24):
    """a small free camera that looks at the sphere from -x, +y (away from the cap and the voxel of weight 0): dict for render_view / render_twin"""
    c = g["centre_vox"] * VS; R = g["radius_vox"] * VS
    fx = 30.0
    eye = c + (R * fx / (0.4 * height)) * np.array([-0.6, 0.5, 0.62])
    return dict(width=width, height=height, intr=np.array([fx, fx, (width - 1) * 0.5, (height - 1) * 0.5]), dist=np.zeros(5), pose=synthetic.look_at_pose(eye, c))


def view_points(cam, depth, dirs):
    """world points of the hits of a depth plane (fp32): eye + depth * ray"""
    import render_twin
    tc = render_twin.camera_from_pose(cam["pose"], cam["intr"], cam["dist"], cam["width"], cam["height"])
    hv, hu = np.nonzero(depth > 0)
    return tc["eye"] + depth[hv, hu, None].astype(np.float64) * dirs[hv, hu], (hv, hu)


def angle(a, b):
    """angle between unit vectors [M, 3], well conditioned near 0 (arccos of the dot product is not)"""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return 2.0 * np.arcsin(np.minimum(1.0, 0.5 * np.sqrt((d * d).sum(-1))))
