"""The cases of the tests of the ray-cast tracking loop (track.cpp track_frame_run): one table of named cases, each with a scene, a
descriptor, a start seed and the branch of the loop it is named for.  test_track_loop_cpu.py runs the twin (track_twin.track, track_rgbd_twin.track_rgbd) on
them with an analytic model and asserts that every trace shows its branch; test_gpu_track_loop.py runs the twin with the device's own ray cast as the model and
holds i3d_track_frame / i3d_track_frame_rgbd / i3d_fusion_track to it.

A model_fn(level, cam, ref) returns (depth, world normal[, intensity]) of the model ray-cast at ref, as track_twin.track takes it.  A world is what a case's
scene gives both modules: dict(kind, scene (the analytic Scene, None for the slab), intr, w, h, vs, truth (world->camera), dist).

STOP_FACTOR: the stop-rule condition.  No step of any twin run of a case has |omega| or |upsilon| within this factor of its threshold, so that a last-bit
difference of a step cannot end a pass an iteration earlier or later; the seeds of the table were chosen for it, and both modules assert it on the runs they use.
"""
import functools
import math

import numpy as np

import fusion_track_cases as F
import helpers
import track_cases
import track_rgbd_twin as rgbd_twin
import track_twin
from intrinsic3d_amd import synthetic

STOP_FACTOR = 2.0
TRACK_BLOCK = 256              # track_kernels.hpp
MIN_INLIERS = track_twin.MIN_INLIERS
BUMPY, DIST, SHIFT = track_cases.BUMPY, track_cases.DIST, track_cases.SHIFT      # the tracking tests' bumps, distortion and negative octant
SMALL, FULL = (96, 72), (160, 120)
FLAT_VS = 1.0 / 256.0          # the slab's voxel size: a power of two, so that (z0 - k) * vs is exact and the stored field is exactly linear in z
FLAT_Z0 = 12.5                 # the slab's zero plane, voxels
FLAT_HALF = 4                  # voxels stored on either side of it

# levels, iterations (None: the default budgets; "first_pass + 1": read from the twin's trace), seed / rot_deg / trans_vox of the start, what the frame keeps.
# seed = (with the analytic model, with the device's ray cast): the two models are different surfaces (the analytic field, its voxel grid), their step sequences
# differ, and the stop-rule condition is a condition on the sequence; where one seed meets it on both, both entries are that seed.  Scanned: of 30 to 120
# seeds per case about one in three meets the condition on a one-level run and fewer with more passes.  The photometric and the fusion cases take a few steps
# per level only (status 1): with their budgets open, no seed of 24 and no stop rule from 1e-6 to 3e-3 met the condition on either model, the passes' first
# steps fall through the thresholds one after the other.
CASES = {
    "one_level": dict(scene="bumpy", size=SMALL, api="track", levels=1, iterations=None, seed=(1, 8), rot_deg=1.0, trans_vox=2.0,
                      branch="status 0 after at least two passes, the last stopping on its first step"),
    "three_levels": dict(scene="bumpy", size=FULL, api="track", levels=3, iterations=[30, 10, 10], seed=(69, 1), rot_deg=2.0, trans_vox=3.0,
                         branch="a pose handed down twice; the 40 x 30 level is no multiple of TRACK_BLOCK"),
    "skipped_middle": dict(scene="bumpy", size=FULL, api="track", levels=3, iterations=[30, 0, 10], seed=(9, 9), rot_deg=2.0, trans_vox=3.0,
                           branch="budget == 0 && l > 0"),
    "zero_finest": dict(scene="bumpy", size=SMALL, api="track", levels=2, iterations=[0, 10], seed=(2, 2), rot_deg=1.0, trans_vox=2.0,
                        branch="the budget == 0 break at level 0: rms_initial == 0, iterations[0] == 0"),
    "zero_all": dict(scene="bumpy", size=SMALL, api="track", levels=2, iterations=[0, 0], seed=(1, 1), rot_deg=1.0, trans_vox=2.0,
                     branch="every budget 0: the pose is the input, status 1"),
    "budget_used": dict(scene="bumpy", size=SMALL, api="track", levels=1, iterations=[3], seed=(1, 1), rot_deg=1.0, trans_vox=2.0,
                        branch="status 1, iterations[0] == 3"),
    "budget_across_passes": dict(scene="bumpy", size=SMALL, api="track", levels=1, iterations="first_pass + 1", seed=(18, 18), rot_deg=1.0, trans_vox=2.0,
                                 branch="the second pass gets exactly one launch pair"),
    "few_inliers_coarse": dict(scene="bumpy", size=SMALL, api="track", levels=2, iterations=None, seed=(2, 3), rot_deg=0.5, trans_vox=1.0, keep="patch16",
                               branch="level 1 has fewer than 64 inliers: status 2, the pose returned bit for bit; with one level the frame registers"),
    "few_inliers_fine": dict(scene="bumpy", size=SMALL, api="track", levels=2, iterations=None, seed=(3, 3), rot_deg=0.5, trans_vox=1.0, keep="even_pixels",
                             branch="status 2 at level 0 after a level that solved: min_pivot_ratio is the one carried into the fresh state"),
    "flat_one_level": dict(scene="flat", size=SMALL, api="track", levels=1, iterations=None, seed=(1, 1), rot_deg=0.5, trans_vox=1.0, branch="status 3"),
    "flat_two_levels": dict(scene="flat", size=SMALL, api="track", levels=2, iterations=None, seed=(1, 1), rot_deg=0.5, trans_vox=1.0,
                            branch="status 3 at level 1, then the !level0_ready cast: rms_initial == 0, inliers > 0, rms_final > 0"),
    "distortion": dict(scene="bumpy", size=SMALL, api="track", levels=1, iterations=None, seed=(18, 18), rot_deg=1.0, trans_vox=2.0, dist=DIST,
                       branch="a distorted camera: the renderer's undistorted rays against the association's forward model, pass after pass"),
    # J = [p x n, n] with p in world coordinates: 400 m from the origin the rotation pivots are ~(400 m / 6 cm)^2 times the translation pivots, so the last
    # pivots fall below 1e-12 trace and the loop reports status 3 at the coarsest level, in the twin and on the device alike
    "distortion_shifted": dict(scene="bumpy", size=SMALL, api="track", levels=2, iterations=None, seed=(1, 1), rot_deg=1.0, trans_vox=2.0, dist=DIST, shift=SHIFT,
                               branch="a distorted camera on a grid far from the origin: status 3 by the lever arm, then the !level0_ready cast"),
    "rgbd": dict(scene="bumpy", size=SMALL, api="rgbd", levels=2, iterations=[2, 3], seed=(1, 1), rot_deg=1.0, trans_vox=2.0, weights=(1.0, 0.1),
                 branch="photo_rms_initial, photo_rms_final, photo_samples"),
    "rgbd_photo_only": dict(scene="bumpy", size=SMALL, api="rgbd", levels=1, iterations=[3], seed=(1, 1), rot_deg=0.5, trans_vox=1.0, weights=(0.0, 1.0),
                            branch="status 2 counts photometric samples (count_col)"),
    "fusion": dict(scene="fusion", size=FULL, api="fusion", levels=2, iterations=[3, 3], seed=(2, 2), rot_deg=1.0, trans_vox=2.0,
                   branch="Fusion.track: the model is Fusion.render"),
}
# few_inliers_coarse's second descriptor: the same frame with one level registers (three steps of it: the 15 x 15 points of the patch on the device's voxel
# model reach the stop rule by a path that an ulp of the cast changes, so the run ends by its budget, status 1)
ONE_LEVEL = dict(levels=1, iterations=[3])
# the second frame of rgbd_photo_only: the luminance is the model's only on a 7 x 7 patch (49 < 64 samples pass max_photo_residual), the depth is whole
STARVED = dict(max_photo_residual=0.5, patch=7, offset=10.0)


# ---- worlds -----------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bumpy_scene(width, height, shift=None):
    """track_cases.scene at the given image size"""
    sc = dict(helpers.small_scene(seed=5, radius_vox=16, K=3, width=width, height=height, levels=1, **BUMPY))
    vs = float(sc["voxel_size"])
    sc["albedo_true"] = sc["scene"].albedo(sc["keys"].astype(np.float64) * vs)
    eye = sc["center"] + 3.1 * sc["scene"].R * np.array([0.35, 0.45, -0.82]) / np.linalg.norm([0.35, 0.45, -0.82])
    sc["truth"] = synthetic.look_at_pose(eye, sc["center"])
    sc["offset"] = np.zeros(3)
    if shift is not None:
        shift = np.asarray(shift, np.int64)
        sc["keys"] = (sc["keys"] + shift[None, :]).astype(np.int32)
        t = shift.astype(np.float64) * vs
        poses = np.array(sc["poses"], np.float64)
        for f in range(len(poses)):
            poses[f, 3:] = poses[f, 3:] - synthetic.aa_to_rotmat(poses[f, :3]) @ t
        sc["poses"] = poses
        tr = np.array(sc["truth"], np.float64); tr[3:] = tr[3:] - synthetic.aa_to_rotmat(tr[:3]) @ t
        sc["truth"] = tr
        sc["offset"] = t
    return sc


@functools.lru_cache(maxsize=None)
def flat_scene(width, height):
    """an axis-aligned slab: voxels (x, y, k) with sdf = (FLAT_Z0 - k) * FLAT_VS, exactly, so the field is linear in z and its gradient is (0, 0, -1 / vs) at every
    point; a camera in front of it (z < z0) looking along +z, tilted"""
    vs = FLAT_VS
    fx = 525.0 * width / 640.0
    intr = np.array([fx, fx, (width - 1) * 0.5, (height - 1) * 0.5])
    dist_m = 0.2
    nx, ny = int(math.ceil(1.3 * width / fx * dist_m / vs)) + 8, int(math.ceil(1.3 * height / fx * dist_m / vs)) + 8
    k0 = int(math.floor(FLAT_Z0)) - FLAT_HALF + 1
    x, y, k = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(k0, k0 + 2 * FLAT_HALF), indexing="ij")
    keys = np.stack([x.ravel(), y.ravel(), k.ravel()], -1).astype(np.int32)
    sdf = (FLAT_Z0 - keys[:, 2].astype(np.float64)) * vs
    n = keys.shape[0]
    centre = np.array([0.5 * nx * vs, 0.5 * ny * vs, FLAT_Z0 * vs])
    eye = centre + dist_m * np.array([0.12, -0.08, -1.0])
    return dict(voxel_size=vs, keys=keys, sdf=sdf, weight=np.ones(n, np.float32), color=np.full((n, 3), 128, np.uint8), albedo_true=np.full(n, 0.6),
                intr=intr, width=width, height=height, center=centre, truth=synthetic.look_at_pose(eye, centre), scene=None)


def world(name):
    c = CASES[name]
    w, h = c["size"]
    dist = np.asarray(c.get("dist", np.zeros(5)), np.float64)
    if c["scene"] == "fusion":
        scene = F.scene()
        return dict(kind="fusion", scene=scene, offset=np.zeros(3), intr=F.INTR.copy(), w=F.W, h=F.H, vs=F.VS, truth=F.arc_pose(scene, 14.0, 24.0), dist=dist, sc=None)
    sc = flat_scene(w, h) if c["scene"] == "flat" else bumpy_scene(w, h, c.get("shift"))
    return dict(kind=c["scene"], scene=sc["scene"], offset=sc.get("offset", np.zeros(3)), intr=np.asarray(sc["intr"], np.float64), w=w, h=h,
                vs=float(sc["voxel_size"]), truth=np.asarray(sc["truth"], np.float64), dist=dist, sc=sc)


# ---- analytic models (no device) ----------------------------------------------------------------------------------------------------------------------------------
def _rays(cam, ref):
    v, u = np.meshgrid(np.arange(cam["h"], dtype=np.float64), np.arange(cam["w"], dtype=np.float64), indexing="ij")
    x, y = track_twin.undistort(cam, u.ravel(), v.ravel())
    R = ref["R"]
    return np.stack([(R[0, a] * x + R[1, a] * y) + R[2, a] for a in range(3)], -1)


def analytic_model(wd, intensity=False):
    """the bumpy sphere marched analytically (track_twin.raycast_scene), or the exact plane z = FLAT_Z0 * FLAT_VS with world normal (0, 0, -1)"""
    def model(level, cam, ref):
        h, w = cam["h"], cam["w"]
        if wd["kind"] == "flat":
            d = _rays(cam, ref)
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (FLAT_Z0 * FLAT_VS - ref["eye"][2]) / d[:, 2]
            hit = np.isfinite(t) & (t > 0)
            depth = np.where(hit, t, 0.0).astype(np.float32).reshape(h, w)
            normal = np.where(hit[:, None], np.array([0.0, 0.0, -1.0]), 0.0).astype(np.float32).reshape(h, w, 3)
            return depth, normal
        shifted = dict(ref, eye=ref["eye"] - wd["offset"])
        depth, normal = track_twin.raycast_scene(wd["scene"], cam, shifted)
        if not intensity:
            return depth, normal
        p = shifted["eye"] + depth.reshape(-1, 1).astype(np.float64) * _rays(cam, ref)
        lum = np.where(depth.reshape(-1) > 0, wd["scene"].shade(p), 0.0).astype(np.float32).reshape(h, w)
        return depth, normal, lum
    return model


def ulp_model(model_fn, seed):
    """model_fn with every non-zero depth and normal component moved by one fp32 ulp, the sign seeded: the reference's own sensitivity to the last bit of a cast"""
    rng = np.random.default_rng(seed)

    def model(level, cam, ref):
        out = list(model_fn(level, cam, ref))
        for i in (0, 1):
            a = np.asarray(out[i], np.float32)
            to = np.where(rng.integers(0, 2, a.shape) == 1, np.float32(np.inf), np.float32(-np.inf))
            out[i] = np.where(a != 0, np.nextafter(a, to), a).astype(np.float32)
        return tuple(out)
    return model


# ---- frames, starts, descriptors, runs ----------------------------------------------------------------------------------------------------------------------------
def start_pose(name, wd, on="analytic", seed=None):
    """the start of a case on the analytic model or on the device's: the truth turned by rot_deg and moved by trans_vox voxels, seeded"""
    c = CASES[name]
    seed = c["seed"][("analytic", "device").index(on)] if seed is None else seed
    return track_twin.perturb(wd["truth"], np.random.default_rng(seed), c["rot_deg"], c["trans_vox"] * wd["vs"])


def make_frame(name, wd, model_fn):
    """the frame of a case: the model cast at the true pose (depth[, luminance]), cut down to what the case keeps"""
    c = CASES[name]
    cam0 = track_twin.level_camera(wd["intr"], wd["dist"], wd["w"], wd["h"], 0)
    out = model_fn(0, cam0, track_twin.ref_from_pose(wd["truth"]))
    depth = np.array(out[0], np.float32)
    lum = np.array(out[2], np.float32) if len(out) > 2 else None
    keep = c.get("keep")
    if keep == "patch16":
        vv, uu = np.nonzero(depth > 0)
        v0, u0 = (int(round(vv.mean())) - 8) // 2 * 2, (int(round(uu.mean())) - 8) // 2 * 2
        cut = np.zeros_like(depth); cut[v0:v0 + 16, u0:u0 + 16] = depth[v0:v0 + 16, u0:u0 + 16]
        depth = cut
    elif keep == "even_pixels":
        cut = np.zeros_like(depth); cut[0::2, 0::2] = depth[0::2, 0::2]
        depth = cut
    return dict(depth=depth, lum=lum)


def starved_frame(fr):
    """rgbd_photo_only's second frame: the depth whole, the luminance off by STARVED["offset"] outside a patch at the middle of the hits"""
    depth, lum = fr["depth"], fr["lum"].copy()
    vv, uu = np.nonzero(depth > 0)
    n = STARVED["patch"]
    v0, u0 = int(round(vv.mean())) - n // 2, int(round(uu.mean())) - n // 2
    off = lum + np.float32(STARVED["offset"]); off[v0:v0 + n, u0:u0 + n] = lum[v0:v0 + n, u0:u0 + n]
    return dict(depth=depth, lum=off)


def descriptor(name, iterations=None, levels=None):
    c = CASES[name]
    it = c["iterations"] if iterations is None else iterations
    assert not isinstance(it, str), "budget_across_passes: pass the budget read from the twin's trace"
    d = track_twin.default_desc(levels=c["levels"] if levels is None else levels, **c.get("desc", {}))
    if it is not None:
        d["iterations"] = list(it) + [0] * (4 - len(it))
    return d


def run_twin(name, wd, fr, start, model_fn, desc, max_photo_residual=0.0):
    """(pose, stats, passes) of the twin's traced run"""
    c = CASES[name]
    if c["api"] == "rgbd":
        wg, wp = c["weights"]
        return rgbd_twin.track_rgbd(fr["depth"], fr["lum"], wd["intr"], wd["dist"], start, model_fn, desc, wg, wp, max_photo_residual, trace=True)
    return track_twin.track(fr["depth"], wd["intr"], wd["dist"], start, model_fn, desc, trace=True)


def twin_case(name, wd, model_fn, on="analytic", seed=None):
    """the case run on the twin: dict(frame, start, desc, pose, stats, passes); budget_across_passes reads its budget from a first run's trace"""
    c = CASES[name]
    fr = make_frame(name, wd, model_fn)
    start = start_pose(name, wd, on, seed)
    if c["iterations"] == "first_pass + 1":
        first = run_twin(name, wd, fr, start, model_fn, descriptor(name, iterations=[30]))[2]
        assert first[0]["status"] == 0 and first[0]["iterations"] > 1, first[0]
        desc = descriptor(name, iterations=[first[0]["iterations"] + 1])
    else:
        desc = descriptor(name)
    pose, st, passes = run_twin(name, wd, fr, start, model_fn, desc)
    return dict(frame=fr, start=start, desc=desc, pose=pose, stats=st, passes=passes, levels_px=levels_px(wd, desc["levels"]))


# ---- what a run must show -----------------------------------------------------------------------------------------------------------------------------------------
def stop_margin(passes, desc):
    """the largest of min(x / thr, thr / x) over every step's |omega| and |upsilon|: 1 is a step on its threshold, <= 1 / STOP_FACTOR is the condition"""
    worst = 0.0
    for p in passes:
        for nw, nu in p["steps"]:
            for x, thr in ((nw, desc["stop_rotation"]), (nu, desc["stop_translation"])):
                worst = max(worst, min(x / thr, thr / x) if x > 0.0 else 0.0)
    return worst


def assert_stop_rule_clear(passes, desc):
    m = stop_margin(passes, desc)
    assert m <= 1.0 / STOP_FACTOR, f"a step lies within a factor {1.0 / m:.2f} of its stop threshold"


def solved(passes):
    return [p for p in passes if p["status"] is not None]


def check_branch(name, run):
    """asserts that the twin's run shows the branch the case is named for"""
    st, passes, start, pose = run["stats"], run["passes"], run["start"], run["pose"]
    it = st["iterations"]
    at = lambda l: [p for p in solved(passes) if p["level"] == l]
    if name == "one_level":
        assert st["status"] == 0 and len(passes) >= 2 and passes[-1]["iterations"] == 1 and passes[-1]["status"] == 0, (st, len(passes))
        assert it[0] == sum(p["iterations"] for p in passes)
    elif name == "three_levels":
        assert [p["level"] for p in passes] == sorted((p["level"] for p in passes), reverse=True) and all(at(l) for l in (2, 1, 0)), passes
        assert at(1)[0]["pose"].tobytes() != at(2)[0]["pose"].tobytes() and at(0)[0]["pose"].tobytes() != at(1)[0]["pose"].tobytes()
        assert run["levels_px"][2] == 40 * 30 and (40 * 30) % TRACK_BLOCK != 0
        assert st["status"] in (0, 1) and all(it[l] > 0 for l in (0, 1, 2)), st
    elif name == "skipped_middle":
        assert at(2) and not at(1) and at(0) and it[1] == 0 and it[2] > 0 and it[0] > 0, st
    elif name == "zero_finest":
        assert at(1) and not at(0) and passes[-1]["level"] == 0 and passes[-1]["status"] is None, passes
        assert st["rms_initial"] == 0.0 and it[0] == 0 and it[1] > 0 and st["rms_final"] > 0.0 and st["status"] == at(1)[-1]["status"], st
    elif name == "zero_all":
        assert not solved(passes) and len(passes) == 1 and st["status"] == 1 and it == [0, 0, 0, 0] and st["rms_initial"] == 0.0 and st["inliers"] > 0, st
    elif name == "budget_used":
        assert st["status"] == 1 and it[0] == 3 and len(passes) == 1, st
    elif name == "budget_across_passes":
        budget = run["desc"]["iterations"][0]
        assert len(passes) == 2 and passes[0]["iterations"] == budget - 1 and passes[0]["status"] == 0 and passes[1]["iterations"] == 1 and it[0] == budget, (st, budget)
    elif name == "few_inliers_coarse":
        assert st["status"] == 2 and len(passes) == 1 and passes[0]["level"] == 1 and passes[0]["inliers"] < MIN_INLIERS, (st, passes[0]["inliers"])
        assert np.asarray(pose).tobytes() == np.asarray(start, np.float64).tobytes() and it == [0, 0, 0, 0]
    elif name == "few_inliers_fine":
        assert st["status"] == 2 and at(1) and at(1)[-1]["status"] in (0, 1) and passes[-1]["level"] == 0 and passes[-1]["inliers"] < MIN_INLIERS, st
        assert np.asarray(pose).tobytes() == np.asarray(start, np.float64).tobytes() and it[0] == 0 and it[1] > 0 and st["min_pivot_ratio"] > 0.0, st
    elif name == "flat_one_level":
        assert st["status"] == 3 and len(passes) == 1 and passes[0]["status"] == 3 and it[0] == 0 and passes[0]["inliers"] >= MIN_INLIERS, st
        assert st["rms_initial"] > 0.0 and st["rms_final"] > 0.0
    elif name == "flat_two_levels":
        assert st["status"] == 3 and len(passes) == 2 and passes[0]["level"] == 1 and passes[0]["status"] == 3 and passes[0]["inliers"] >= MIN_INLIERS, st
        assert passes[1]["level"] == 0 and passes[1]["status"] is None and st["rms_initial"] == 0.0 and st["inliers"] > 0 and st["rms_final"] > 0.0, st
    elif name == "distortion":
        assert st["status"] == 0 and len(at(0)) >= 2 and passes[-1]["iterations"] == 1, st
    elif name == "fusion":
        assert st["status"] == 1 and it == [3, 3, 0, 0] and len(at(1)) == 1 and len(at(0)) == 1 and st["rms_final"] < st["rms_initial"], st
    elif name == "distortion_shifted":
        assert st["status"] == 3 and len(passes) == 2 and passes[0]["level"] == 1 and passes[0]["status"] == 3 and passes[0]["inliers"] >= MIN_INLIERS, st
        assert passes[1]["status"] is None and st["rms_initial"] == 0.0 and st["rms_final"] > 0.0 and 0.0 < st["min_pivot_ratio"] < 1e-11, st
    elif name == "rgbd":
        assert st["status"] == 1 and it == [2, 3, 0, 0] and st["photo_samples"] > MIN_INLIERS and st["photo_rms_initial"] > st["photo_rms_final"] > 0.0, st
    elif name == "rgbd_photo_only":
        assert st["status"] == 1 and it[0] == 3 and st["photo_samples"] > MIN_INLIERS and st["photo_rms_initial"] > st["photo_rms_final"] > 0.0, st
    else:
        raise AssertionError(name)
    if st["status"] == 3:
        assert np.abs(np.asarray(pose) - np.asarray(start)).max() <= 1e-12
        assert 0.0 <= st["min_pivot_ratio"] <= 1.0 and math.isfinite(st["min_pivot_ratio"])


def levels_px(wd, levels):
    return [track_twin.level_camera(wd["intr"], wd["dist"], wd["w"], wd["h"], l)["w"] * track_twin.level_camera(wd["intr"], wd["dist"], wd["w"], wd["h"], l)["h"]
            for l in range(levels)]


def failing_pivot(tot):
    """(1e-12 * trace / pmax, column) of the first pivot of track_twin.solve's factorisation that fails d > 1e-12 trace, pmax the largest pivot up to and including
    that column: the bound on min_pivot_ratio of a status 3 (inf when no pivot up to there is > 0, where the ratio is 0 by definition)"""
    tot = [float(x) for x in tot]
    A = [[0.0] * 6 for _ in range(6)]
    for k, (a, c) in enumerate(track_twin.UPPER):
        A[a][c] = A[c][a] = tot[k]
    trace = A[0][0]
    for a in range(1, 6):
        trace = trace + A[a][a]
    L = [[0.0] * 6 for _ in range(6)]
    piv = []
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d = d - L[j][k] * L[j][k]
        piv.append(d)
        if not d > 1e-12 * trace:
            pm = max(piv)
            return (1e-12 * trace / pm if pm > 0.0 else math.inf), j
        L[j][j] = math.sqrt(d)
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v = v - L[i][k] * L[j][k]
            L[i][j] = v / L[j][j]
    raise AssertionError("no pivot fails")
