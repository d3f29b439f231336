"""The device's ray-cast tracking loop (track.cpp track_frame_run: i3d_track_frame, i3d_track_frame_rgbd, i3d_fusion_track) held to its twin run for run on the
cases of track_loop_cases.py.  The twin runs with the device's own ray cast as its model (render_view / Fusion.render at each pass's pose), so what is compared
is the loop: budgets across passes, the carried min_pivot_ratio, rms_initial, the level end, the status mapping, the budget == 0 branches, the cast after a
degenerate coarser level.  Status, iteration counts and valid_pixels are exact; inliers may flip on 0.1 % of the pixels (the allowance of
test_gpu_track.py::test_sums_match_twin); the pose bar of a case is measured on the twin alone: 100 x the pose difference of two more twin runs whose model
planes are moved by one fp32 ulp (the later casts of the twin go through cw_to_pose and can differ from the driver's by that much), floor 1e-12.  Also: status 3
and the defined min_pivot_ratio through the shared solve's other drivers (register_points, track_frame_sdf) on the flat slab.

rms_initial and photo_rms_initial: 1e-9 relative where level 0 is the first level that iterates (cast and association at the start pose); where a coarser level
ran first they are figures on a later cast and are held as rms_final is.  Measured on an MI355X with level 0 given no budget, so that the pose after level 1 is
what returns: the device's and the twin's poses agree to 1.3e-15 rad and rms_final, on the level-0 cast at that pose, to 3.9e-9 relative - the same 3.9e-9 by
which rms_initial of the rgbd case (budgets [2, 3]) differs.  The depth-only tracker shows the same (6.8e-9 after one step at level 1).

Measured on an MI355X (DESIGN.md 14.4 has the table): every case agrees with the twin 4 to 9 orders of magnitude inside its pose bar.  Before the photometric
term set a coordinate within 1e-9 pixel of a pixel centre to that centre the rgbd case ended 5.9e-5 rad from its twin, min_pivot_ratio
3.8e-3 off: the side of a bilinear cell corner fell to the last bit of a projection."""
import functools
import math

import numpy as np
import pytest

import fusion_track_cases
import query_twin
import register_twin as RT
import track_cases
import track_loop_cases as LC
import track_sdf_twin as ST
import track_twin
from intrinsic3d_amd import binding

pytestmark = pytest.mark.gpu

FLIPS = 0.001                 # of the level-0 pixel count


def open_model(name, wd):
    """the device object of a case's world: a Context with the grid (and the scene's SH for the photometric cases), or the fused volume"""
    c = LC.CASES[name]
    if wd["kind"] == "fusion":
        return fusion_track_cases.fused(wd["scene"])
    sc = wd["sc"]
    if wd["kind"] == "flat":
        ctx = binding.Context(0)
        ctx.set_grid(sc["voxel_size"], sc["keys"], sc["sdf"], sc["sdf"], sc["albedo_true"], sc["weight"], sc["color"])
        return ctx
    return track_cases.rgbd_context(sc, c.get("dist"), sh=c["api"] == "rgbd")


def device_model(obj, api, start=None):
    """model_fn over the device's own ray cast.  The cast at the start pose is given that pose as it is (the driver's first cast: the same R and eye); every
    other cast goes through cw_to_pose"""
    first = track_twin.pose_to_cw(start) if start is not None else None

    def model(level, cam, ref):
        if first is not None and np.array_equal(ref["R"], first[0].T) and np.array_equal(ref["eye"], first[1]):
            pose = np.asarray(start, np.float64)
        else:
            pose = track_twin.cw_to_pose(ref["R"].T, ref["eye"])
        camera = dict(width=cam["w"], height=cam["h"], intr=cam["intr"], dist=cam["dist"], pose=pose)
        if api == "fusion":
            out = obj.render(camera=camera, planes=("depth", "normal"))
            return out["depth"], out["normal"]
        planes = ("depth", "normal", "intensity") if api == "rgbd" else ("depth", "normal")
        out = obj.render_view(frame=-1, planes=planes, camera=camera)
        return tuple(out[k] for k in planes)
    return model


def device_track(obj, name, wd, fr, start, desc, max_photo_residual=0.0):
    c = LC.CASES[name]
    kw = dict(levels=desc["levels"], iterations=list(desc["iterations"]), dist=wd["dist"], stop_rotation=desc["stop_rotation"], stop_translation=desc["stop_translation"])
    if c["api"] == "fusion":
        return obj.track(fr["depth"], start, wd["intr"], **kw)
    if c["api"] == "rgbd":
        wg, wp = c["weights"]
        return obj.track_frame_rgbd(fr["depth"], fr["lum"], start, intr=wd["intr"], geometric_weight=wg, photo_weight=wp, max_photo_residual=max_photo_residual, **kw)
    return obj.track_frame(fr["depth"], start, intr=wd["intr"], **kw)


@functools.lru_cache(maxsize=None)
def _case(name):
    """the case on the twin (the device's cast as the model), on the twin with the model planes moved by an ulp (twice), and on the device (twice); extras for
    the cases with a second frame or descriptor"""
    wd = LC.world(name)
    obj = open_model(name, wd)
    try:
        api = LC.CASES[name]["api"]
        start = LC.start_pose(name, wd, "device")
        model = device_model(obj, api, start)
        run = LC.twin_case(name, wd, model, "device")
        assert np.array_equal(run["start"], start)
        moved = [LC.run_twin(name, wd, run["frame"], start, LC.ulp_model(model, seed), run["desc"]) for seed in (1, 2)]
        dev = [device_track(obj, name, wd, run["frame"], start, run["desc"]) for _ in range(2)]
        extra = {}
        if name == "few_inliers_coarse":
            d1 = LC.descriptor(name, **LC.ONE_LEVEL)
            extra = dict(desc=d1, twin=LC.run_twin(name, wd, run["frame"], start, model, d1), dev=device_track(obj, name, wd, run["frame"], start, d1),
                         moved=[LC.run_twin(name, wd, run["frame"], start, LC.ulp_model(model, seed), d1) for seed in (1, 2)])
        if name == "rgbd_photo_only":
            fr = LC.starved_frame(run["frame"]); mr = LC.STARVED["max_photo_residual"]
            extra = dict(twin=LC.run_twin(name, wd, fr, start, model, run["desc"], mr), dev=device_track(obj, name, wd, fr, start, run["desc"], mr))
    finally:
        obj.close()
    return dict(wd=wd, run=run, moved=moved, dev=dev, extra=extra)


def pose_bar(run, moved, vs):
    """(rad, voxel) bars: 100 x the larger pose difference of the moved twin runs to the unmoved one, floor 1e-12; the moved runs take the same path"""
    ang = tr = 0.0
    for pose, st, passes in moved:
        assert st["status"] == run["stats"]["status"] and st["iterations"] == run["stats"]["iterations"], (st, run["stats"])
        a, t = ST.pose_err(pose, run["pose"], vs)
        ang, tr = max(ang, a), max(tr, t)
    return max(100.0 * ang, 1e-12), max(100.0 * tr, 1e-12, translation_floor(run["pose"], vs)), (ang, tr)


def translation_floor(pose6, vs):
    """what pose_err's second figure cannot resolve, in voxels.  A pose holds t = -R c; a component of t takes three products and two sums to form and as many
    to turn back into the centre, about 5 roundings of half an ulp of the largest |t| per pose and axis, two poses, three axes: 5 * sqrt(3) < 16 ulps.  Near the
    origin that is far below the floor of 1e-12 voxel; 400 m away (distortion_shifted) an ulp of t is 1.4e-11 voxel"""
    return 16.0 * float(np.spacing(np.abs(np.asarray(pose6, np.float64)[3:]).max())) / vs


def compare(label, wd, desc, twin, dev, bars):
    """the device's (pose, stats) against the twin's (pose, stats, passes)"""
    (pose_t, st_t, passes), (pose_d, st_d) = twin, dev
    bar_ang, bar_tr, _ = bars
    px = wd["w"] * wd["h"]
    ang, tr = ST.pose_err(pose_d, pose_t, wd["vs"])
    print(f"{label}: status {st_d['status']} iterations {st_d['iterations']} bar {bar_ang:.3e} rad {bar_tr:.3e} voxel, observed {ang:.3e} rad {tr:.3e} voxel; "
          f"inliers {st_d['inliers']} / {st_t['inliers']}, rms_final {st_d['rms_final']:.9e} / {st_t['rms_final']:.9e}, "
          f"min_pivot_ratio {st_d['min_pivot_ratio']:.9e} / {st_t['min_pivot_ratio']:.9e}")
    assert st_d["status"] == st_t["status"], (st_d, st_t)
    assert list(st_d["iterations"]) == list(st_t["iterations"]), (st_d, st_t)
    assert st_d["valid_pixels"] == st_t["valid_pixels"], (st_d, st_t)
    assert abs(st_d["inliers"] - st_t["inliers"]) <= FLIPS * px, (st_d, st_t)
    # rms_initial is the first association of level 0.  Where level 0 is the first level that iterates, cast and association are at the start pose and only the
    # order of the sums differs: 1e-9.  Where a coarser level ran first it is taken on a later cast, which the twin makes through cw_to_pose and which differs from
    # the driver's in the last bit of some fp32 depths; it is then held as the other figure on a later cast is, rms_final: the translation bar + 1e-6 of its value
    at_start = passes[0]["level"] == 0 or st_t["rms_initial"] == 0.0
    first = (lambda v: 1e-9 * v) if at_start else (lambda v: bar_tr * wd["vs"] + 1e-6 * v)
    assert abs(st_d["rms_initial"] - st_t["rms_initial"]) <= first(st_t["rms_initial"]), (st_d["rms_initial"], st_t["rms_initial"], at_start)
    assert abs(st_d["rms_final"] - st_t["rms_final"]) <= bar_tr * wd["vs"] + 1e-6 * st_t["rms_final"], (st_d["rms_final"], st_t["rms_final"])
    if "photo_samples" in st_t:
        print(f"    photo_samples {st_d['photo_samples']} / {st_t['photo_samples']}, photo_rms_initial {st_d['photo_rms_initial']:.9e} / {st_t['photo_rms_initial']:.9e}, "
              f"photo_rms_final {st_d['photo_rms_final']:.9e} / {st_t['photo_rms_final']:.9e}")
        assert abs(st_d["photo_samples"] - st_t["photo_samples"]) <= FLIPS * px, (st_d, st_t)
        assert abs(st_d["photo_rms_initial"] - st_t["photo_rms_initial"]) <= first(st_t["photo_rms_initial"]), (st_d["photo_rms_initial"], st_t["photo_rms_initial"], at_start)
        assert abs(st_d["photo_rms_final"] - st_t["photo_rms_final"]) <= bar_tr * wd["vs"] + 1e-6 * st_t["photo_rms_final"]
    if st_t["status"] == 2:
        assert np.asarray(pose_d).tobytes() == np.asarray(pose_t, np.float64).tobytes()          # the pose as it came in
    else:
        assert ang <= bar_ang and tr <= bar_tr, (ang, bar_ang, tr, bar_tr)
    r_d, r_t = st_d["min_pivot_ratio"], st_t["min_pivot_ratio"]
    assert math.isfinite(r_d) and 0.0 <= r_d <= 1.0
    if st_t["status"] != 3:
        assert abs(r_d - r_t) <= 1e-6 * r_t, (r_d, r_t)
    else:
        failing = [p for p in passes if p["status"] == 3]
        assert len(failing) == 1 and failing[0]["iterations"] == 0                                  # its first association is the system that failed
        bound, column = LC.failing_pivot(failing[0]["sums"][:29])
        print(f"    status 3 at column {column}: min_pivot_ratio bound {bound:.3e}")
        assert r_d <= bound and r_t <= bound
        assert abs(r_d - r_t) <= (1e-6 * bound if math.isfinite(bound) else 0.0), (r_d, r_t, bound)


@pytest.mark.parametrize("name", list(LC.CASES))
def test_loop_matches_twin(name):
    c = _case(name)
    wd, run = c["wd"], c["run"]
    LC.check_branch(name, run)
    LC.assert_stop_rule_clear(run["passes"], run["desc"])
    for _, _, passes in c["moved"]:
        LC.assert_stop_rule_clear(passes, run["desc"])
    bars = pose_bar(run, c["moved"], wd["vs"])
    compare(name, wd, run["desc"], (run["pose"], run["stats"], run["passes"]), c["dev"][0], bars)
    (p0, s0), (p1, s1) = c["dev"]
    assert np.asarray(p0).tobytes() == np.asarray(p1).tobytes() and s0 == s1                        # a second call returns the same bits
    if name == "zero_all":                                                                          # no step: the input pose to the round trip of the conversion
        assert np.abs(np.asarray(p0) - run["start"]).max() <= 1e-12


def test_few_inliers_coarse_succeeds_with_one_level():
    c = _case("few_inliers_coarse")
    pose, st, passes = c["extra"]["twin"]
    assert st["status"] == 1 and st["iterations"][0] == 3 and passes[0]["inliers"] >= LC.MIN_INLIERS and st["rms_final"] < st["rms_initial"], st
    LC.assert_stop_rule_clear(passes, c["extra"]["desc"])
    for _, _, moved in c["extra"]["moved"]:
        LC.assert_stop_rule_clear(moved, c["extra"]["desc"])
    wd = c["wd"]
    run = dict(c["run"], pose=pose, stats=st)
    compare("few_inliers_coarse, levels 1", wd, c["extra"]["desc"], c["extra"]["twin"], c["extra"]["dev"], pose_bar(run, c["extra"]["moved"], wd["vs"]))


def test_photo_only_status_2_counts_photometric_samples():
    c = _case("rgbd_photo_only")
    pose_t, st_t, passes = c["extra"]["twin"]
    pose_d, st_d = c["extra"]["dev"]
    print(st_d, st_t)
    assert st_t["status"] == 2 and st_t["inliers"] >= LC.MIN_INLIERS and 0 < st_t["photo_samples"] < LC.MIN_INLIERS, st_t
    assert st_d["status"] == 2 and st_d["inliers"] >= LC.MIN_INLIERS and st_d["photo_samples"] == st_t["photo_samples"] and st_d["inliers"] == st_t["inliers"], st_d
    assert np.asarray(pose_d).tobytes() == np.asarray(c["run"]["start"], np.float64).tobytes() == pose_t.tobytes()
    assert list(st_d["iterations"]) == [0, 0, 0, 0] and st_d["valid_pixels"] == st_t["valid_pixels"]


# ---- the flat slab under the shared solve's other drivers -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _slab():
    """the slab on the device: its depth frame (the device's cast at the true pose), the start, the results of track_frame_sdf and register_points and their twins"""
    name = "flat_one_level"
    wd = LC.world(name)
    sc = wd["sc"]
    grid = query_twin.Grid(sc["keys"], sc["sdf"], sc["weight"], wd["vs"], albedo=sc["albedo_true"])
    start = LC.start_pose(name, wd, "device")
    obj = open_model(name, wd)
    try:
        depth = LC.make_frame(name, wd, device_model(obj, "track"))["depth"]
        sdf_dev = [obj.track_frame_sdf(depth, start, intr=wd["intr"], dist=wd["dist"]) for _ in range(2)]
        pts, ok, _ = ST.samples(depth, wd["intr"], wd["dist"])
        pose_cw = RT.rt_to_pose(*ST.pose_to_cw(start))
        reg_dev = [obj.register_points(pts[ok], pose_cw) for _ in range(2)]
    finally:
        obj.close()
    sdf_twin = ST.track(grid, depth, wd["intr"], wd["dist"], start, trace=True)
    reg_twin = RT.register(grid, pts[ok], pose_cw, trace=True)
    return dict(start=start, pose_cw=pose_cw, sdf_dev=sdf_dev, sdf_twin=sdf_twin, reg_dev=reg_dev, reg_twin=reg_twin)


def _degenerate(label, given, dev, twin):
    (pose_d, st_d), (pose_d2, st_d2) = dev
    pose_t, st_t = twin
    bound, column = LC.failing_pivot(st_t["trace"][0]["sums"])
    print(f"{label}: device {st_d}\n    twin status {st_t['status']} min_pivot_ratio {st_t['min_pivot_ratio']:.3e}, failing column {column}, bound {bound:.3e}")
    assert st_t["status"] == 3 and st_t["iterations"] == 0 and st_t["inliers"] >= LC.MIN_INLIERS
    assert st_d["status"] == 3 and st_d["iterations"] == 0 and st_d["inliers"] == st_t["inliers"] and st_d["valid"] == st_t["valid"], (st_d, st_t)
    assert np.asarray(pose_d).tobytes() == np.asarray(given, np.float64).tobytes() == np.asarray(pose_t).tobytes()          # no step: the pose as it came in
    r_d, r_t = st_d["min_pivot_ratio"], st_t["min_pivot_ratio"]
    assert math.isfinite(r_d) and 0.0 <= r_d <= 1.0 and r_d <= bound and r_t <= bound
    assert abs(r_d - r_t) <= (1e-6 * bound if math.isfinite(bound) else 0.0), (r_d, r_t, bound)
    assert abs(st_d["rms_initial"] - st_t["rms_initial"]) <= 1e-9 * st_t["rms_initial"]
    assert np.asarray(pose_d2).tobytes() == np.asarray(pose_d).tobytes() and st_d2 == st_d


def test_slab_is_status_3_for_track_frame_sdf():
    s = _slab()
    _degenerate("track_frame_sdf on the slab", s["start"], s["sdf_dev"], s["sdf_twin"])


def test_slab_is_status_3_for_register_points():
    s = _slab()
    _degenerate("register_points on the slab", s["pose_cw"], s["reg_dev"], s["reg_twin"])
