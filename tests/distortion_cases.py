"""The scenes of the tests that hold the solver's rows to the oracle OFF the zero point of the lens distortion and at keyframes with a zero or
near-zero rotation (test_oracle_cpu.py asserts their input conditions on the oracle alone, test_gpu_distortion.py compares the device on them).

Every other solver scene comes from synthetic.make_scene with dist = 0 and cameras that orbit the object.  At k = 0 the distortion's part of the chain
rule multiplies by zero (build.hip: dcr, the k3 / k4 parts of dxd_dx0 .. dyd_dy0, c2 = 2 k4 y0 of the five distortion partials; xd = x0 in the intrinsics
partials), the float observation pass skips its Brown branch (camera.cpp:135), and an orbiting camera never meets the first-order branch of the angle-axis
rotation (frame_math.hpp: |w|^2 <= DBL_EPSILON) nor its neighbourhood.

Base scene: helpers.small_scene(seed=10, radius_vox=9, K=6, width=96, height=72); 6640 voxels after helpers.oracle_setup.
Distortions: DIST (the vector of test_gpu_cull.py and tools/jacobian_vs_oracle.py), STRONG = 3 DIST, and BELOW, whose entries all lie under the float
pass's threshold 1e-5: a solve started there is assembled without the Brown branch in its first iteration and with it in the second.
Small-rotation keyframes: keyframes 0, 1, 2 replaced by cameras at eye = center - (0, 0, d), d = keyframe 0's distance from the centre, with the angle-axis
vectors SMALL_AA: the first-order branch at exactly zero, the same branch at a non-zero vector, and the Rodrigues branch just above the switch
(|w|^2 = 5e-16 > DBL_EPSILON = 2.2e-16).  Pose = [aa, -R(aa) eye]; the frame is rendered again.  The float poses of keyframes 0 and 1 are equal, so their
observation weights tie exactly: which of them survives the top-5 cut is std::sort's doing (colorization.cpp:357-370; test_oracle_cpu.py states the rule).

Measured on the oracle: DIST gives 8560 Eg rows (1348 .. 1507 per keyframe), zero distortion 9086 rows on another (voxel, keyframe) set."""
import functools

import numpy as np

import helpers
from intrinsic3d_amd import synthetic

DIST = np.array([0.08, -0.03, 0.002, 0.003, -0.002])
STRONG = 3.0 * DIST
BELOW = np.array([9e-6, 0.0, 0.0, -9e-6, 9e-6])
FLOAT_PASS_THRESHOLD = 1e-5                 # camera.cpp:135 (Eigen isZero): the Brown branch is taken when any |k| exceeds it
SMALL_AA = np.array([[0.0, 0.0, 0.0], [1e-9, 0.0, 0.0], [2e-8, -1e-8, 0.0]])
REPLACED = (0, 1, 2)

# name: (distortion, keyframes 0..2 replaced)
CASES = {
    "distorted": (DIST, False),
    "strong": (STRONG, False),
    "small_rotations": (np.zeros(5), True),
    "both": (DIST, True),
}
GROUPS = (("sdf", 0, 10), ("albedo", 10, 14), ("pose", 14, 20), ("intrinsics", 20, 24), ("distortion", 24, 29))

MIN_ROWS = 1000
MIN_ROWS_PER_REPLACED = 200


@functools.lru_cache(maxsize=None)
def _base():
    return helpers.small_scene(seed=10, radius_vox=9, K=6, width=96, height=72)


def scene(dist, small_rotations=False):
    """A copy of the base scene with the distortion set and, if asked, keyframes 0, 1, 2 replaced (the base scene itself is never changed)."""
    sc = dict(_base())
    sc["dist"] = np.array(dist, np.float64)
    if small_rotations:
        poses = np.array(sc["poses"], np.float64); frames = list(sc["frames"])
        R0 = synthetic.aa_to_rotmat(poses[0, :3])
        d = float(np.linalg.norm(-R0.T @ poses[0, 3:] - sc["center"]))
        eye = sc["center"] - np.array([0.0, 0.0, d])
        rng = np.random.default_rng(0)
        for k, aa in zip(REPLACED, SMALL_AA):
            poses[k] = np.concatenate([aa, -synthetic.aa_to_rotmat(aa) @ eye])
            lum, depth, bgr = synthetic.render_frame(sc["scene"], poses[k], sc["intr"], sc["width"], sc["height"], 0.0, rng, None)
            frames[k] = {"lum": [lum], "depth": [depth], "bgr": [bgr]}
        sc["poses"] = poses; sc["frames"] = frames
    return sc


def case_scene(name):
    dist, small = CASES[name]
    return scene(dist, small)


def row_set(pv):
    """(the Eg rows of a ProblemView without Jacobian, their (voxel, keyframe) set)"""
    rows = pv.eg(with_jacobian=False)
    return rows, set(zip(rows[0].tolist(), rows[1].tolist()))


def input_facts(O, name, sc, g, fr, vsh, ocfg, pv):
    """What a case must exercise, measured on the oracle: the number of Eg rows, the rows of each replaced keyframe (None: orbiting cameras), and whether the
    (voxel, keyframe) set differs from the one the oracle builds on the same scene at zero distortion (None: the case has no distortion)."""
    dist, small = CASES[name]
    (v, f, _, _, _), rows = row_set(pv)
    facts = dict(rows=len(v), per_keyframe=np.bincount(f, minlength=sc["K"]).tolist(), replaced=None, moved=None)
    if small:
        facts["replaced"] = [int(np.sum(f == k)) for k in REPLACED]
    if np.any(dist != 0.0):
        pv0 = O.ProblemView(g, fr, ocfg, sc["intr"], np.zeros(5), sc["poses"], vsh, 0)
        _, rows0 = row_set(pv0)
        pv0.free()
        facts["moved"] = len(rows ^ rows0)
        facts["rows_at_zero"] = len(rows0)
    return facts


def jacobian_figures(J, Jg):
    """The two checks of test_gpu_parity.test_eg_residual_and_jacobian on the rows handed in, as error over tolerance per column group (<= 1 passes): `entry`, the
    worst |Jg - J| / (1e-4 |J| + 2e-6 x the column's largest |J| over THESE rows); `row`, the worst error relative to the row's largest partial of the group, over 2e-4, on
    the rows whose group scale exceeds 1e-2 of the group's largest column maximum.  A group whose columns are all zero (no such partial on these rows) reports 0."""
    J = np.asarray(J, np.float64); Jg = np.asarray(Jg, np.float64)
    colmax = np.abs(J).max(axis=0, keepdims=True)
    tol = 1e-4 * np.abs(J) + 2e-6 * colmax
    err = np.abs(Jg - J)
    over = np.where(tol > 0.0, err / np.where(tol > 0.0, tol, 1.0), np.where(err > 0.0, np.inf, 0.0))
    out = {}
    for name, lo, hi in GROUPS:
        sc = np.abs(J[:, lo:hi]).max(axis=1, keepdims=True) + 1e-30
        big = sc[:, 0] > 1e-2 * colmax[0, lo:hi].max()
        rel = float((err[big, lo:hi] / sc[big]).max()) if big.any() else 0.0
        out[name] = dict(entry=float(over[:, lo:hi].max()), row=rel / 2e-4, rows=int(big.sum()))
    return out


def assert_inputs(name, facts):
    dist, small = CASES[name]
    assert facts["rows"] > MIN_ROWS, facts
    if small:
        assert min(facts["replaced"]) >= MIN_ROWS_PER_REPLACED, facts
    if np.any(dist != 0.0):
        assert np.any(np.abs(dist) > FLOAT_PASS_THRESHOLD) and facts["moved"] > 0, facts
