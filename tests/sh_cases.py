"""Grids for the SH stage tests: the smallest shapes at which the lighting kernels can go wrong.  Each is handed over with set_grid;
no frames, no camera.  A case is a dict: grid (as tests/sh_twin.py takes it), size (subvolume size, 0 = one global volume), thres, and what it was built to hold.

"runs", "single" and "ineligible" keep the fp32 part of the features independent of whether a compiler fuses multiply-adds: the voxel size is 2^-8 m, sdf_refined
is an integer multiple of Q = 2^-13 m with |k| <= 60 (every difference, square and sum of squares is then exact in fp32; sqrtf and the division round correctly
either way), thres_shell = 2 voxels = 64 Q, a colour has exactly one non-zero channel (the luminance has one rounding), the albedo is random in [0.3, 1].
"awkward" keeps the same sdf and colour conditions at voxel size 0.004 m, where the subvolume arithmetic is inexact."""
import functools

import numpy as np

import sh_twin

Q = 2.0 ** -13
VS = 2.0 ** -8
SIZE = 2.0 ** -3            # 32 voxels
THRES = 64 * Q              # = 2 * VS
# eligible voxels per subvolume, x index -3 .. 2; between them: 0 between two non-empty ones, 1, 63 / 64 / 65 (a tile), 2047 / 2048 / 2049 (a chunk), 4096 / 4097
RUN_LENGTHS = ((2049, 4097, 0, 4096, 64, 1), (2047, 4096, 65, 0, 2048, 63))


def _block(x, y, z):
    g = np.meshgrid(np.arange(*x), np.arange(*y), np.arange(*z), indexing="ij")
    return np.stack([a.ravel() for a in g], axis=1).astype(np.int32)


def _fields(rng, keys, vs, k=None):
    n = keys.shape[0]
    k = rng.integers(-60, 61, n) if k is None else k
    color = np.zeros((n, 3), np.uint8)
    color[np.arange(n), rng.integers(0, 3, n)] = rng.integers(1, 256, n)
    sdf = k.astype(np.float64) * Q
    return dict(voxel_size=vs, keys=keys, sdf=sdf.copy(), sdf_refined=sdf, albedo=rng.uniform(0.3, 1.0, n), weight=np.ones(n, np.float32), color=color)


@functools.lru_cache(maxsize=None)
def runs(arrangement):
    """The block x in [-80, 80), y in [-32, 0), z in [-6, 0): six subvolumes in a row (x index -3 .. 2, so S % 4 = 2), the number of eligible voxels of each
    set to RUN_LENGTHS[arrangement] by zeroing the albedo of the surplus."""
    rng = np.random.default_rng(100 + arrangement)
    keys = _block((-80, 80), (-32, 0), (-6, 0)); keys = keys[rng.permutation(keys.shape[0])]
    grid = _fields(rng, keys, VS)
    el = sh_twin.eligible(grid, THRES)
    ix = sh_twin.subvolume_index(keys, VS, SIZE)[:, 0]
    for s, want in enumerate(RUN_LENGTHS[arrangement]):
        cand = np.nonzero(el & (ix == s - 3))[0]
        assert cand.size >= want
        grid["albedo"][rng.permutation(cand)[want:]] = 0.0
    return dict(name=f"runs{arrangement}", grid=grid, size=SIZE, thres=THRES, run_lengths=RUN_LENGTHS[arrangement])


@functools.lru_cache(maxsize=None)
def single():
    """the first "runs" grid as one global volume: one run of all its eligible voxels (five chunks and 67 voxels: a full tile and a partial one)"""
    c = runs(0)
    return dict(name="single", grid=c["grid"], size=0.0, thres=THRES)


INELIGIBLE = ("weight0", "weight0_px", "weight0_py", "weight0_pz", "missing_px", "missing_py", "missing_pz", "above_thres", "at_thres", "flat",
              "albedo_zero", "albedo_negative_zero", "albedo_nan")


@functools.lru_cache(maxsize=None)
def ineligible():
    """The block x in [-20, 32), y, z in [0, 4).  Probe k sits at (4 k + 1 - 20, 1, 1) and fails eligibility in the k-th way of INELIGIBLE ("at_thres" passes:
    |sdf| == thres is inside the shell); the probes are four voxels apart, so each defect stays with its probe and the voxels whose forward neighbour it is."""
    rng = np.random.default_rng(7)
    keys = _block((-20, 32), (0, 4), (0, 4))
    grid = _fields(rng, keys, VS)
    pos = {tuple(k): i for i, k in enumerate(keys.tolist())}
    probes = {}; drop = []
    for k, what in enumerate(INELIGIBLE):
        t = (4 * k + 1 - 20, 1, 1); i = pos[t]; probes[what] = t
        fwd = [pos[(t[0] + 1, t[1], t[2])], pos[(t[0], t[1] + 1, t[2])], pos[(t[0], t[1], t[2] + 1)]]
        if what == "weight0": grid["weight"][i] = 0.0
        elif what.startswith("weight0_"): grid["weight"][fwd["xyz".index(what[-1])]] = 0.0
        elif what.startswith("missing_"): drop.append(fwd["xyz".index(what[-1])])
        elif what == "above_thres": grid["sdf_refined"][i] = 65 * Q
        elif what == "at_thres": grid["sdf_refined"][i] = -64 * Q
        elif what == "flat": grid["sdf_refined"][fwd] = grid["sdf_refined"][i]
        elif what == "albedo_zero": grid["albedo"][i] = 0.0
        elif what == "albedo_negative_zero": grid["albedo"][i] = -0.0
        elif what == "albedo_nan": grid["albedo"][i] = np.nan
    keep = np.ones(keys.shape[0], bool); keep[drop] = False
    keep = np.nonzero(keep)[0][rng.permutation(int(keep.sum()))]
    grid = {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in grid.items()}
    return dict(name="ineligible", grid=grid, size=SIZE, thres=THRES, probes=probes)


AWKWARD_SIZES = (0.05, 0.035)


@functools.lru_cache(maxsize=None)
def awkward(size):
    """The shell (2.2 voxels to either side) of a sphere at voxel size 0.004, its sdf quantised to Q and cut to |k| <= 60, centred at (12.5, 2.3, -1.7) voxels so
    that the keys and the subvolume indices take both signs in all three coordinates.  The radius is 13 voxels: a key of 25 is the smallest besides 0 whose
    (float(c) * vs) * (1 / 0.05) comes within rounding of an integer (0.004 / 0.05 = 2 / 25), and the floor must be tested where rounding decides it."""
    vs = 0.004; rng = np.random.default_rng(21)
    centre = np.array([12.5, 2.3, -1.7]); radius = 13.0
    keys = _block((-4, 30), (-14, 19), (-18, 15))
    d = np.linalg.norm(keys - centre, axis=1) - radius
    m = np.abs(d) <= 2.2
    keys = keys[m]; d = d[m]
    p = rng.permutation(keys.shape[0]); keys = keys[p]; d = d[p]
    k = np.clip(np.rint(d * vs / Q), -60, 60).astype(np.int64)
    grid = _fields(rng, keys, vs, k)
    return dict(name=f"awkward{size}", grid=grid, size=size, thres=2.0 * vs)


def all_cases():
    return [runs(0), runs(1), single(), ineligible()] + [awkward(s) for s in AWKWARD_SIZES]


@functools.lru_cache(maxsize=None)
def twin_stages(name):
    """the twin's statement of a case, computed once and shared (read-only) by the tests"""
    c = {c["name"]: c for c in all_cases()}[name]
    st = sh_twin.stages(c["grid"], c["size"], c["thres"])
    for v in st.values():
        v.setflags(write=False)
    return st
