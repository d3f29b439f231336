"""i3d_render_view on the device: against the analytic scene, against its numpy statement (render_twin.py), and what it must leave alone."""

import numpy as np
import pytest

import helpers
import render_twin
from intrinsic3d_amd import binding, synthetic

pytestmark = pytest.mark.gpu

ALL = binding.RENDER_PLANES
DIST = helpers.TRACK_DIST


def _scene(shift=None, levels=1, seed=5):
    sc = dict(helpers.small_scene(seed=seed, radius_vox=12, K=3, width=96, height=72, levels=levels))
    vs = float(sc["voxel_size"])
    P = sc["keys"].astype(np.float64) * vs
    sc["albedo_true"] = sc["scene"].albedo(P)
    if shift is not None:                            # the same scene in the negative octant, far from the origin (world shifted by t: tr' = tr - R t)
        shift = np.asarray(shift, np.int64)
        sc["keys"] = (sc["keys"] + shift[None, :]).astype(np.int32)
        t = shift.astype(np.float64) * vs
        poses = np.array(sc["poses"], np.float64)
        for f in range(len(poses)):
            poses[f, 3:] = poses[f, 3:] - synthetic.aa_to_rotmat(poses[f, :3]) @ t
        sc["poses"] = poses
    return sc


def _context(sc, sdf_refined=None, albedo=None, dist=None):
    n = sc["keys"].shape[0]
    ctx = binding.Context(0)
    ctx.set_grid(sc["voxel_size"], sc["keys"], sc["sdf"], sc["sdf"] if sdf_refined is None else sdf_refined,
                 sc["albedo_true"] if albedo is None else albedo, sc["weight"], sc["color"])
    ctx.set_frames(sc["frames"], sc["levels"])
    ctx.set_camera(sc["intr"], np.zeros(5) if dist is None else dist, sc["poses"])
    assert ctx.N == n
    return ctx


def _perturbed(sc, seed=11):
    rng = np.random.default_rng(seed)
    vs = float(sc["voxel_size"]); n = sc["keys"].shape[0]
    sdf_r = sc["sdf"].astype(np.float64) + rng.normal(0.0, 0.05 * vs, n)
    alb = sc["albedo_true"] + rng.normal(0.0, 0.01, n)
    return sdf_r, alb


def _twin_cam(ctx, frame, level, sc):
    intr, dist, poses = ctx.get_camera()
    h, w = sc["frames"][frame]["lum"][level].shape
    return render_twin.camera_from_pose(poses[frame], intr * 0.5 ** level, dist, w, h)


def _twin_grid(ctx, refined=True, sh=True):
    a = ctx.export_grid()
    _, vs, _ = ctx.grid_info()
    return render_twin.Grid(a["keys"], a["sdf_refined"] if refined else a["sdf"], a["weight"], vs, albedo=a["albedo"],
                            sh=ctx.get_voxel_sh() if sh else None), vs


def _compare(dev, tw, cam, vs, lum=None):
    hd, ht = dev["depth"] > 0, tw["hit"]
    assert ht.sum() > 200
    assert (hd != ht).sum() <= 0.002 * ht.sum(), ((hd & ~ht).sum(), (ht & ~hd).sum(), ht.sum())
    common = hd & ht
    dd = np.abs(dev["depth"].astype(np.float64) - tw["depth"])[common]
    assert np.quantile(dd, 0.999) <= 1e-3 * vs and dd.max() <= 0.05 * vs, (np.quantile(dd, 0.999) / vs, dd.max() / vs)
    same = common & (np.abs(dev["depth"] - tw["depth"]) <= 1e-3 * vs)           # the pixels whose march took the same path
    if "normal" in dev:
        dot = np.clip((dev["normal"].astype(np.float64) * tw["normal"]).sum(-1), -1.0, 1.0)[same]
        assert np.arccos(dot).max() <= 1e-3
    for k in ("albedo", "shading", "intensity"):
        if k in dev:
            assert np.abs(dev[k] - tw[k])[same].max() <= 1e-4, k
            assert np.all(dev[k][~hd] == 0.0)
    if "residual" in dev:
        assert np.array_equal(dev["residual"][hd], (dev["intensity"] - lum)[hd]) and np.all(dev["residual"][~hd] == 0.0)
    hv, hu = np.nonzero(common)
    pu, pv = render_twin.project(cam, cam["eye"] + dev["depth"][hv, hu, None].astype(np.float64) * tw["dir"][hv, hu])
    assert np.abs(pu - hu).max() < 1e-3 and np.abs(pv - hv).max() < 1e-3
    assert dev["stats"]["hits"] == int(hd.sum()) and dev["stats"]["samples"] > 0


def test_render_analytic_sphere():
    """fused SDF of the bump-free sphere, true albedo and SH: depth, normal and intensity against synthetic.render_frame"""
    sc = dict(helpers.small_scene(seed=3, radius_vox=16, K=4, bump_amp_vox=0.0))
    vs = float(sc["voxel_size"]); scene = sc["scene"]
    sc["albedo_true"] = scene.albedo(sc["keys"].astype(np.float64) * vs)
    ctx = _context(sc)
    try:
        ctx.set_voxel_sh(np.tile(synthetic.SH_TRUE, (ctx.N, 1)))
        for f in range(sc["K"]):
            out = ctx.render_view(frame=f, level=0, refined=False, planes=("depth", "normal", "intensity"))
            lum, depth = synthetic.render_frame(scene, sc["poses"][f], sc["intr"], sc["width"], sc["height"])[:2]
            inner = _erode(depth > 0, 2) & _erode(out["depth"] > 0, 2)
            assert inner.sum() > 500
            dd = np.abs(out["depth"].astype(np.float64) - depth)[inner]
            assert np.median(dd) <= 0.05 * vs and dd.max() <= 0.5 * vs, (np.median(dd) / vs, dd.max() / vs)
            cam = render_twin.camera_from_pose(sc["poses"][f], sc["intr"], np.zeros(5), sc["width"], sc["height"])
            d = render_twin.rays(cam)[0].reshape(sc["height"], sc["width"], 3)
            n_ref = scene.normal(cam["eye"] + depth[..., None].astype(np.float64) * d)
            ang = np.degrees(np.arccos(np.clip((out["normal"] * n_ref).sum(-1), -1.0, 1.0)))[inner]
            assert np.median(ang) <= 2.0, np.median(ang)
            assert np.median(np.abs(out["intensity"] - lum)[inner]) <= 0.01
    finally:
        ctx.close()


def _erode(m, r):
    out = m.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out &= np.roll(np.roll(m, dy, 0), dx, 1)
    return out


CASES = {"level0": dict(level=0), "level1_distortion": dict(level=1, levels=2, dist=DIST),
         "negative_octant": dict(level=0, shift=(-100000, -99987, -100021)), "fused_sdf": dict(level=0, refined=False)}


@pytest.mark.parametrize("case", list(CASES))
def test_render_matches_twin(case):
    kw = CASES[case]
    sc = _scene(shift=kw.get("shift"), levels=kw.get("levels", 1))
    sdf_r, alb = _perturbed(sc)
    ctx = _context(sc, sdf_r, alb, dist=kw.get("dist"))
    try:
        vs = float(sc["voxel_size"])
        ctx.estimate_sh(0.05, 10.0, 2.0 * vs)
        refined = kw.get("refined", True)
        grid, _ = _twin_grid(ctx, refined)
        level = kw["level"]
        for f in range(sc["K"]):
            h, w = sc["frames"][f]["lum"][level].shape
            lum = ctx.get_frame_image(f, level, w, h)[0]
            dev = ctx.render_view(frame=f, level=level, refined=refined, planes=ALL)
            cam = _twin_cam(ctx, f, level, sc)
            tw = render_twin.render(grid, cam, lum=lum)
            _compare(dev, tw, cam, vs, lum)
            rms = np.sqrt(dev["stats"]["residual_sq_sum"] / dev["stats"]["hits"])
            assert abs(rms - np.sqrt(np.mean(dev["residual"][dev["depth"] > 0].astype(np.float64) ** 2))) <= 1e-5
    finally:
        ctx.close()


def test_custom_camera_equals_keyframe():
    sc = _scene(levels=2)
    sdf_r, alb = _perturbed(sc)
    ctx = _context(sc, sdf_r, alb, dist=DIST)
    try:
        ctx.estimate_sh(0.05, 10.0, 2.0 * float(sc["voxel_size"]))
        intr, dist, poses = ctx.get_camera()
        planes = ("depth", "normal", "albedo", "shading", "intensity")
        for f in range(sc["K"]):
            h, w = sc["frames"][f]["lum"][1].shape
            a = ctx.render_view(frame=f, level=1, planes=planes)
            b = ctx.render_view(frame=-1, planes=planes, camera=dict(width=w, height=h, intr=intr * 0.5, dist=dist, pose=poses[f]))
            assert (a["depth"] > 0).sum() > 100
            for k in planes:
                assert np.array_equal(a[k], b[k]), k
            assert a["stats"] == b["stats"]
    finally:
        ctx.close()


def test_brick_cache_follows_the_grid():
    sc = _scene()
    ctx = _context(sc)
    try:
        planes = ("depth", "normal", "albedo")
        first = ctx.render_view(frame=0, planes=planes)
        ctx.upsample()
        _, vs, _ = ctx.grid_info()
        ctx.clear_outside_thin_shell(2.0 * vs)
        out = ctx.render_view(frame=0, planes=planes)
        grid, vs = _twin_grid(ctx, sh=False)
        assert abs(vs - 0.5 * float(sc["voxel_size"])) < 1e-9
        cam = _twin_cam(ctx, 0, 0, sc)
        _compare(out, render_twin.render(grid, cam), cam, vs)
        assert out["stats"]["samples"] != first["stats"]["samples"]
    finally:
        ctx.close()


def test_rendering_changes_nothing():
    sc = _scene(seed=9)
    sdf_r, alb = _perturbed(sc)
    vs = float(sc["voxel_size"])
    cfg = binding.default_config(iterations=1, thres_shell=2.0 * vs)
    results = []
    for render in (False, True):
        ctx = _context(sc, sdf_r, alb)
        try:
            ctx.estimate_sh(0.05, 10.0, 2.0 * vs)
            stats = []
            for _ in range(2):
                if render:
                    for f in range(sc["K"]):
                        ctx.render_view(frame=f, planes=ALL)
                stats += ctx.optimize(cfg)
            results.append((ctx.export_grid(), ctx.get_camera(), stats))
        finally:
            ctx.close()
    (g0, c0, s0), (g1, c1, s1) = results
    for k in g0:
        assert np.array_equal(g0[k], g1[k]), k
    for a, b in zip(c0, c1):
        assert np.array_equal(a, b)
    for a, b in zip(s0, s1):
        for name, _ in binding.IterationStats._fields_:
            if not name.startswith("time_"):
                x, y = getattr(a, name), getattr(b, name)
                assert (list(x) == list(y)) if hasattr(x, "__len__") else x == y, name


def test_render_errors():
    sc = _scene()
    cam = dict(width=32, height=24, intr=[30.0, 30.0, 15.5, 11.5], dist=np.zeros(5), pose=sc["poses"][0])
    with binding.Context(0) as ctx:
        with pytest.raises(binding.I3DError):
            ctx.render_view(frame=0)
        with pytest.raises(binding.I3DError):
            ctx.render_view(frame=-1, camera=cam, planes=("depth",))
        ctx.set_grid(sc["voxel_size"], sc["keys"], sc["sdf"], sc["sdf"], sc["albedo_true"], sc["weight"], sc["color"])
        with pytest.raises(binding.I3DError):
            ctx.render_view(frame=0, planes=("depth",))                 # no keyframes / camera
        ctx.set_frames(sc["frames"], sc["levels"])
        ctx.set_camera(sc["intr"], np.zeros(5), sc["poses"])
        with pytest.raises(binding.I3DError):
            ctx.render_view(frame=sc["K"], planes=("depth",))
        with pytest.raises(binding.I3DError):
            ctx.render_view(frame=0, level=sc["levels"], planes=("depth",))
        with pytest.raises(binding.I3DError):
            ctx.render_view(frame=0, planes=("shading",))               # no SH yet
        with pytest.raises(binding.I3DError):
            ctx.render_view(frame=-1, camera=cam, planes=("residual",))
        with pytest.raises(binding.I3DError):
            ctx.render_view(frame=-1, camera=dict(cam, width=0), planes=("depth",))
        full = ctx.render_view(frame=1, planes=("depth", "normal", "albedo"))
        only = ctx.render_view(frame=1, planes=())
        assert set(only) == {"stats"} and only["stats"]["hits"] == full["stats"]["hits"] == int((full["depth"] > 0).sum()) > 0
        near = ctx.render_view(frame=1, planes=("depth",), depth_range=(float(full["depth"][full["depth"] > 0].max()) + 1e-3, 0.0))
        assert near["stats"]["hits"] == 0
