"""The numpy statement of i3d_fusion_register_volume (register_volume_twin.py) on hand-made volumes, no device: the selection against a
brute-force statement, convergence back to a known motion from three starts, the two summation orders, `limit`, and the empty selection.

The volumes are a bumpy sphere (radius 12 voxels, bumps of 12 voxels as in register_cases: with query_cases' half-voxel bumps a rotation is hardly observable)
sampled at the lattice points within +-5 voxels of its surface, in fusion_merge_twin.volume() form.  B is the same field resampled on a lattice moved by a known
rigid motion T (x_A = R x_B + t), so register(A, B) must come back to T up to the interpolation error of the trilinear field."""
import math

import numpy as np
import pytest

import fusion_deintegrate_twin as DT
import fusion_merge_twin as MT
import query_twin as QT
import register_volume_twin as VT
from intrinsic3d_amd import synthetic

VS = float(np.float32(0.004))
RADIUS_VOX, BUMP_VOX, BAND_VOX = 12.0, 12.0, 5.0
CENTRE = np.array([3.3, -2.6, 5.1]) * VS                       # the shell's keys straddle zero on every axis
SCENE = synthetic.Scene(CENTRE, RADIUS_VOX * VS, BUMP_VOX * VS, 40.0)
AXIS = np.array([0.3, -0.8, 0.52])
T_TRUE = np.concatenate([AXIS / np.linalg.norm(AXIS) * math.radians(7.0), np.array([2.3, -1.7, 3.1]) * VS])
# the trilinear interpolant of a field with second derivatives up to amp f^2 + 2 / radius is off by at most h^2 / 8 times the sum over the axes of that
INTERP_ERR = 3.0 * (VS * VS / 8.0) * (BUMP_VOX * VS * 40.0 * 40.0 + 2.0 / (RADIUS_VOX * VS))


def _volume(pose6=None):
    """the field at the lattice points k of a world moved by pose6 (x_scene = R k vs + t), where it is within the band"""
    half = int(RADIUS_VOX + BUMP_VOX + BAND_VOX + 8)
    ax = np.arange(-half, half + 1, dtype=np.int64)
    k = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3) + np.round(CENTRE / VS).astype(np.int64)
    p = k.astype(np.float64) * VS
    if pose6 is not None:
        R, t = VT.pose_to_rt(pose6)
        p = p @ R.T + t
    s = SCENE.sdf(p)
    on = np.abs(s) <= BAND_VOX * VS
    rng = np.random.default_rng(7)
    perm = rng.permutation(int(on.sum()))                                 # a volume has no order of its own
    return MT.volume(k[on][perm], s[on][perm].astype(np.float32), np.ones(int(on.sum()), np.float32))


@pytest.fixture(scope="module")
def volumes():
    A, B = _volume(), _volume(T_TRUE)
    return A, B, QT.Grid(A["keys"], A["sdf"].astype(np.float64), A["weight"], VS)


@pytest.mark.parametrize("stride", [1, 2, 3])
def test_selection_is_the_brute_force_statement(volumes, stride):
    A, _, _ = volumes
    A = dict(A); A["weight"] = A["weight"].copy(); A["weight"][::17] = 0.0; A["sdf"] = A["sdf"].copy(); A["sdf"][5::23] = np.nan
    sel = VT.select(A, VS, 2.0, stride)
    band = 2.0 * VS
    want = []
    for k, s, w in zip(A["keys"].tolist(), A["sdf"].tolist(), A["weight"].tolist()):
        if w != 0 and abs(s) <= band and all(c == stride * math.floor(c / stride) for c in k):
            want.append((((k[2] + (1 << 20)) << 42) | ((k[1] + (1 << 20)) << 21) | (k[0] + (1 << 20)), k, s))
    want.sort()
    assert len(want) > 100 and (A["keys"] < 0).any(0).all() and (A["keys"] > 0).any(0).all()
    assert np.array_equal(sel["keys"], np.array([w[1] for w in want], np.int64))
    assert np.array_equal(sel["sdf"], np.array([w[2] for w in want], np.float32))
    assert np.array_equal(sel["points"], sel["keys"].astype(np.float64) * VS)
    assert any(c < 0 for w in want for c in w[1])                        # negative multiples of the stride are there
    assert np.all(np.diff(DT.pack(sel["keys"])) > 0)


STARTS = [(0, 1.0, 1.5), (1, 1.2, 1.2), (2, 0.8, 1.6)]


def _start(seed, deg, vox):
    rng = np.random.default_rng(100 + seed)
    a = rng.normal(size=3); a *= math.radians(deg) / np.linalg.norm(a)
    u = rng.normal(size=3); u *= vox * VS / np.linalg.norm(u)
    R, t = VT.pose_to_rt(T_TRUE)
    dR = synthetic.aa_to_rotmat(a)
    c = CENTRE                                                           # the perturbation turns about the object, not about the origin
    return VT.rt_to_pose(dR @ R, dR @ (t - c) + c + u)


def test_registers_back_to_the_known_motion(volumes):
    A, B, grid = volumes
    found = []
    for seed, deg, vox in STARTS:
        start = _start(seed, deg, vox)
        d0 = VT.pose_diff(start, T_TRUE, VS)
        pose, st = VT.register(grid, B, VS, start)
        ang, tr = VT.pose_diff(pose, T_TRUE, VS)
        print(f"start {seed}: {math.degrees(d0[0]):.3f} deg / {d0[1]:.3f} voxel off -> status {st['status']} after {st['iterations']} steps, "
              f"{math.degrees(ang):.5f} deg / {tr:.5f} voxel off, {st['selected']} selected, {st['valid']} valid, {st['inliers']} inliers, "
              f"rms {st['rms_initial']:.3e} -> {st['rms_final']:.3e} m")
        assert st["status"] == 0 and 0 < st["iterations"] < 30
        assert st["selected"] > 3000 and st["inliers"] > 0.9 * st["selected"]
        assert st["rms_final"] < st["rms_initial"] and st["rms_final"] <= INTERP_ERR
        # a shift of the whole field by e changes r by |grad f| e ~ e: the fit cannot be further off than the interpolation error, nor turn by more than that
        # over the radius
        assert tr * VS <= INTERP_ERR and ang <= INTERP_ERR / (RADIUS_VOX * VS)
        found.append(pose)
    for p in found[1:]:                                                  # one minimum: the starts meet within what the stop rule leaves
        ang, tr = VT.pose_diff(p, found[0], VS)
        assert ang < 1e-4 and tr * VS < 1e-4


def test_sequential_and_pairwise_agree(volumes):
    A, B, grid = volumes
    start = _start(0, 1.0, 1.5)
    sel = VT.select(B, VS)
    R, t = VT.pose_to_rt(start)
    c = VT.pivot(grid, sel, start)
    a = VT.sums(grid, sel, R, t - c, c, 0.05)
    b = VT.sums(grid, sel, R, t - c, c, 0.05, order="sequential")
    assert (a["valid"], a["inliers"]) == (b["valid"], b["inliers"]) and a["inliers"] > 3000
    assert np.all(np.abs(a["sums"] - b["sums"]) <= a["n"] * 2.0 ** -52 * a["abs_sums"])
    pa, sa = VT.register(grid, B, VS, start)
    pb, sb = VT.register(grid, B, VS, start, order="sequential")
    ang, tr = VT.pose_diff(pa, pb, VS)
    print(f"sequential against pairwise: {ang:.3e} rad, {tr:.3e} voxel")
    assert (sa["status"], sa["iterations"]) == (sb["status"], sb["iterations"]) == (0, sa["iterations"])
    assert ang < 1e-10 and tr < 1e-8


def test_limit_takes_the_first_entries_in_key_order(volumes):
    A, B, grid = volumes
    sel = VT.select(B, VS)
    R, t = VT.pose_to_rt(T_TRUE)
    c = VT.pivot(grid, sel, T_TRUE)
    for m in (1, 63, 65, 257):
        head = dict(keys=sel["keys"][:m], sdf=sel["sdf"][:m], points=sel["points"][:m])
        a = VT.sums(grid, sel, R, t - c, c, 0.05, limit=m)
        b = VT.sums(grid, head, R, t - c, c, 0.05)
        assert a["n"] == m and a["valid"] == b["valid"] and np.array_equal(a["sums"], b["sums"])
    assert VT.sums(grid, sel, R, t - c, c, 0.05, limit=0)["n"] == len(sel["keys"]) == VT.sums(grid, sel, R, t - c, c, 0.05, limit=10 ** 9)["n"]


def test_empty_selection_is_status_2_with_the_pose_untouched(volumes):
    A, B, grid = volumes
    start = _start(1, 1.2, 1.2)
    for src, desc in ((MT.volume(), {}), (B, dict(source_band_voxels=1e-9)), (B, dict(stride=61))):
        pose, st = VT.register(grid, src, VS, start, desc)
        assert st["status"] == 2 and st["iterations"] == 0 and st["selected"] == 0 and np.array_equal(pose, start) and pose is not start
    pose, st = VT.register(QT.Grid(np.zeros((0, 3), np.int64), np.zeros(0), np.zeros(0, np.float32), VS), B, VS, start)      # nothing to register against
    assert st["status"] == 2 and st["selected"] > 0 and st["valid"] == 0 and np.array_equal(pose, start)
