"""i3d_query_points / i3d_fusion_query_points on the device: against the numpy statement (query_twin.py) on the point sets of
query_cases.py, against the renderer, the reproducible stats, the fusion volume against the context of its export, what the calls must leave alone, and the errors."""
import ctypes as C

import numpy as np
import pytest

import fusion_cases as FC
import helpers
import query_cases as Q
import query_twin as T
import render_twin
from fusion_cases import fusion_frames  # noqa: F401  (fixture)
from intrinsic3d_amd import binding as B

pytestmark = pytest.mark.gpu

VS = Q.VS
SIZES = (1, 63, 65, 257)
STAT_SUMS = ("sum_abs_sdf", "sum_sq_sdf", "sum_abs_distance", "sum_sq_distance")
STAT_EXACT = ("valid", "projected", "steps", "max_abs_sdf", "max_abs_distance")


@pytest.fixture(scope="module")
def contexts():
    """one context per grid of query_cases.GRIDS, created on first use"""
    made = {}

    def get(name):
        if name not in made:
            g = Q.GRIDS[name]()
            ctx = B.Context(0)
            ctx.set_grid(VS, g["keys"], g["sdf"], g["sdf_refined"], g["albedo"], g["weight"], g["color"])
            made[name] = ctx
        return made[name]
    yield get
    for ctx in made.values():
        ctx.close()


def _ulp_equal(a, b):
    """fp32 arrays equal or one ulp apart"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.all(np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64))


def _check_stats(dev, tw):
    for k in STAT_EXACT:
        assert dev[k] == tw[k], (k, dev[k], tw[k])
    for k in STAT_SUMS:                                           # the device's order of summation is not numpy's
        assert abs(dev[k] - tw[k]) <= 1e-12 * abs(tw[k]), (k, dev[k], tw[k])


def _check_values(out, tw, sl=slice(None)):
    assert np.array_equal(out["status"] & 1, tw["status"][sl] & 1)
    tol = 32.0 * 2.0 ** -52 * tw["corner_max"][sl]                # 8 products of three factors and 7 additions
    assert np.all(np.abs(out["sdf"] - tw["sdf"][sl]) <= tol)
    assert _ulp_equal(out["normal"], tw["normal"][sl]) and _ulp_equal(out["albedo"], tw["albedo"][sl])
    off = (out["status"] & 1) == 0
    assert not out["sdf"][off].any() and not out["normal"][off].any() and not out["albedo"][off].any()
    return np.array_equal(out["sdf"], tw["sdf"][sl]) and np.array_equal(out["normal"], tw["normal"][sl]) and np.array_equal(out["albedo"], tw["albedo"][sl])


@pytest.mark.parametrize("name,refined", [("plain", True), ("plain", False), ("shifted", True), ("negative", True)])
def test_value_query_equals_twin(contexts, name, refined):
    g = Q.GRIDS[name]()
    ctx = contexts(name)
    pts = Q.value_points(g, 31)
    tw = T.query(Q.twin_grid(g, refined), pts, project=False)
    assert (tw["status"] == 1).sum() > 2500 and (tw["status"] == 0).sum() > 400
    bit_equal = True
    for n in SIZES + (pts.shape[0],):
        # the last n points hold the special cases (non-finite, huge, q = -0.5, the cells around the voxel of weight 0), the first n the band
        for sl in (slice(0, n), slice(pts.shape[0] - n, pts.shape[0])):
            out = ctx.query_points(pts[sl], refined=refined, project=0)
            assert set(out) == {"sdf", "normal", "albedo", "status", "stats"} and out["sdf"].shape == (n,)
            bit_equal &= _check_values(out, tw, sl)
            assert out["stats"]["valid"] == int((tw["status"][sl] & 1).sum()) and out["stats"]["projected"] == 0 and out["stats"]["steps"] == 0
    print(f"value query {name} refined={refined}: bit-equal to the twin: {bit_equal}")


@pytest.mark.parametrize("i", range(len(Q.PROJECTION_SETS)))
def test_projection_equals_twin(contexts, i):
    g, refined, pts, tw = Q.projection_set(i)
    ctx = contexts(Q.PROJECTION_SETS[i][0])
    out = ctx.query_points(pts, refined=refined)
    assert np.array_equal(out["status"], tw["status"]) and np.all(out["status"] == 3)
    e_foot = np.abs(out["foot"] - tw["foot"]).max() / VS
    e_dist = np.abs(out["distance"] - tw["distance"]).max() / VS
    print(f"projection set {i}: foot {e_foot:.3e} voxel, distance {e_dist:.3e} voxel, steps {out['stats']['steps']} (twin {tw['stats']['steps']}), "
          f"bit-equal: {np.array_equal(out['foot'], tw['foot']) and np.array_equal(out['distance'], tw['distance'])}")
    assert e_foot <= 1e-9 and e_dist <= 1e-9
    _check_values(out, tw)
    assert out["stats"]["steps"] == tw["stats"]["steps"] and out["stats"]["projected"] == pts.shape[0]
    for n in SIZES:                                               # partial waves and workgroups
        part = ctx.query_points(pts[:n], refined=refined)
        for k in ("sdf", "normal", "albedo", "foot", "distance", "status"):
            assert np.array_equal(part[k], out[k][:n]), (n, k)


def test_projection_cases(contexts):
    g = Q.plain()
    ctx = contexts("plain")
    grid = Q.twin_grid(g)
    # outside every valid cell | a walk that leaves the stored band
    far = (g["centre_vox"] + np.array([[0.0, 0.0, 0.0], [40.0, 3.0, -2.0], [0.0, g["radius_vox"] + 6.0, 0.0]])) * VS
    cap = Q.cap_points(g, 100, 21)
    pts = np.concatenate([far, cap])
    tw = T.query(grid, pts)
    out = ctx.query_points(pts)
    assert np.array_equal(out["status"], tw["status"])
    assert not out["status"][:3].any() and np.all(out["status"][3:] == 1)
    assert not out["foot"].any() and not out["distance"].any() and not out["sdf"][:3].any()
    assert out["sdf"][3:].min() > 0.0 and out["stats"]["steps"] == tw["stats"]["steps"] >= 100
    _check_stats(out["stats"], tw["stats"])
    # already on the surface: the feet of a projection are converged points
    _, _, p0, tw0 = Q.projection_set(0)
    feet = ctx.query_points(p0)["foot"]
    on = ctx.query_points(feet)
    assert np.all(on["status"] == 3) and not on["distance"].any() and np.array_equal(on["foot"], feet) and on["stats"]["steps"] == 0
    assert np.abs(on["sdf"]).max() <= 1e-6 * VS
    # max_steps = 0: only such points have a foot
    both = np.concatenate([p0[:500], feet[:500]])
    tz = T.query(grid, both, max_steps=0)
    oz = ctx.query_points(both, max_steps=0)
    assert np.array_equal(oz["status"], tz["status"]) and np.all(oz["status"][500:] == 3) and ((oz["status"][:500] & 2) != 0).sum() < 5
    assert oz["stats"]["steps"] == 0 and oz["stats"]["projected"] == int(((tz["status"] & 2) != 0).sum())
    # a looser tolerance and a step limit that some points do not meet
    tl = T.query(grid, p0, max_steps=1, tolerance_voxels=1e-3)
    ol = ctx.query_points(p0, max_steps=1, tolerance_voxels=1e-3)
    assert np.array_equal(ol["status"], tl["status"]) and 0 < ((tl["status"] & 2) != 0).sum() < p0.shape[0]
    assert np.abs(ol["foot"] - tl["foot"]).max() <= 1e-9 * VS


def test_query_agrees_with_the_renderer(contexts):
    g = Q.plain()
    ctx = contexts("plain")
    grid = Q.twin_grid(g)
    cam = Q.view_camera(g)
    tc = render_twin.camera_from_pose(cam["pose"], cam["intr"], cam["dist"], cam["width"], cam["height"])
    rt = render_twin.render(grid, tc)
    # the bar: the query twin on the render twin's hits (depth cast to fp32, as the device returns it), x 10
    tp, (tv, tu) = Q.view_points(cam, rt["depth"].astype(np.float32), rt["dir"])
    tq = T.query(grid, tp, project=False)
    assert np.all(tq["status"] == 1)
    bar_sdf = 10.0 * np.abs(tq["sdf"]).max()
    bar_ang = 10.0 * Q.angle(rt["normal"][tv, tu].astype(np.float32), tq["normal"]).max()
    dev = ctx.render_view(frame=-1, camera=cam, planes=("depth", "normal"))
    assert dev["stats"]["hits"] > 250
    pts, (hv, hu) = Q.view_points(cam, dev["depth"], rt["dir"])
    out = ctx.query_points(pts, project=0)
    assert np.all(out["status"] == 1)
    e_sdf = np.abs(out["sdf"]).max()
    e_ang = Q.angle(dev["normal"][hv, hu], out["normal"]).max()
    print(f"view: |sdf| {e_sdf / VS:.3e} voxel (bar {bar_sdf / VS:.3e}), angle {e_ang:.3e} rad (bar {bar_ang:.3e}) over {hv.size} hits")
    assert e_sdf <= bar_sdf and e_ang <= bar_ang


def test_stats(contexts):
    g = Q.plain()
    ctx = contexts("plain")
    _, _, p0, _ = Q.projection_set(0)
    pts = np.concatenate([Q.value_points(g, 31), p0, Q.cap_points(g, 100, 21)])
    tw = T.query(Q.twin_grid(g), pts)
    a = ctx.query_points(pts)
    b = ctx.query_points(pts)
    assert 0 < tw["stats"]["projected"] < tw["stats"]["valid"] < pts.shape[0]
    _check_stats(a["stats"], tw["stats"])
    b0, b1 = (a["status"] & 1) != 0, (a["status"] & 2) != 0
    assert a["stats"]["max_abs_sdf"] == np.abs(a["sdf"][b0]).max() and a["stats"]["max_abs_distance"] == np.abs(a["distance"][b1]).max()
    assert a["stats"] == b["stats"]                                # bit-identical: the sums are formed in a fixed order
    for k in B.QUERY_OUTPUTS:
        assert np.array_equal(a[k], b[k]), k
    only = ctx.query_points(pts, outputs=())                      # stats alone
    assert set(only) == {"stats"} and only["stats"] == a["stats"]
    for n in SIZES:                                               # tail lanes contribute zeros
        part = ctx.query_points(pts[-n:])
        _check_stats(part["stats"], T.query(Q.twin_grid(g), pts[-n:])["stats"])
    empty = ctx.query_points(np.zeros((0, 3)))
    assert not any(empty["stats"].values()) and empty["sdf"].shape == (0,)


# ---- the fusion volume -------------------------------------------------------------------------------------------------------------------------------
FUSION_OUTPUTS = ("sdf", "normal", "foot", "distance", "status")


def _same(a, b):
    for k in FUSION_OUTPUTS:
        assert np.array_equal(a[k], b[k], equal_nan=False), k
    assert a["stats"] == b["stats"]


@pytest.mark.parametrize("correct", [0, 10])
def test_fusion_query_equals_context_query(fusion_frames, correct):
    scene, frames, pts = fusion_frames
    f = FC.fused(frames)
    try:
        before = f.query_points(pts)
        assert set(before) == set(FUSION_OUTPUTS) | {"stats"}
        assert before["stats"]["projected"] > 500 and before["stats"]["valid"] < pts.shape[0]
        assert before["stats"]["sum_abs_distance"] / before["stats"]["projected"] < 1.6 * VS
        f.finish(correct)
        after = f.query_points(pts)
        if correct == 0:
            _same(before, after)                                   # finish(0) leaves the table as it was
        ctx = helpers.context_of_fusion(f, VS)
        try:
            for refined in (False, True):                          # the volume has one field: use_refined_sdf is ignored there
                _same(after, ctx.query_points(pts, outputs=FUSION_OUTPUTS, refined=refined))
                _same(after, f.query_points(pts, refined=refined))
            v_f = f.query_points(pts[:65], project=0); v_c = ctx.query_points(pts[:65], outputs=("sdf", "normal", "status"), refined=False, project=0)
            for k in ("sdf", "normal", "status"):
                assert np.array_equal(v_f[k], v_c[k]), k
            assert v_f["stats"] == v_c["stats"]
        finally:
            ctx.close()
    finally:
        f.close()


def test_queries_change_nothing(contexts, fusion_frames):
    g = Q.plain()
    ctx = contexts("plain")
    cam = Q.view_camera(g)
    planes = ("depth", "normal", "albedo")
    grid0 = ctx.export_grid()
    view0 = ctx.render_view(frame=-1, camera=cam, planes=planes)
    pts = np.concatenate([Q.value_points(g, 31), Q.projection_set(0)[2]])
    for kw in (dict(), dict(refined=False), dict(project=0)):
        ctx.query_points(pts, **kw)
    grid1 = ctx.export_grid()
    view1 = ctx.render_view(frame=-1, camera=cam, planes=planes)
    for k in grid0:
        assert np.array_equal(grid0[k], grid1[k]), k
    for k in planes:
        assert np.array_equal(view0[k], view1[k]), k
    assert view0["stats"] == view1["stats"]
    _, frames, fpts = fusion_frames
    out = []
    for query in (None, fpts):
        f = FC.fused(frames, query)
        try:
            if query is not None:
                f.query_points(query)
            f.finish(10)
            if query is not None:
                f.query_points(query)
            out.append(f.export())
        finally:
            f.close()
    for k in ("keys", "sdf", "weight", "color"):
        assert np.array_equal(out[0][k], out[1][k]), k


def test_errors(contexts, fusion_frames):
    L = B.load()
    pts = np.zeros((4, 3)); sdf = np.zeros(4); foot = np.zeros((4, 3)); dist = np.zeros(4)
    p = B._p

    def desc(**kw):
        return B.query_desc_default(**kw)
    d = desc()
    assert (d.use_refined_sdf, d.project, d.max_steps, d.tolerance_voxels) == (1, 1, 16, 1e-6)
    assert L.i3d_query_points(None, d, 4, p(pts), None, None, None, None, None, None, None) == 1
    assert L.i3d_fusion_query_points(None, d, 4, p(pts), None, None, None, None, None, None) == 1
    with B.Context(0) as empty:
        assert L.i3d_query_points(empty.h, d, 4, p(pts), None, None, None, None, None, None, None) == 4
        assert "no grid" in L.i3d_last_error(empty.h).decode()
    _, frames, _ = fusion_frames
    f = FC.fused(frames[:1])
    try:
        ctx = contexts("plain")
        models = ((lambda dd, n, pp, s_, ft, ds, st: L.i3d_query_points(ctx.h, dd, n, pp, s_, None, None, ft, ds, None, st), lambda: L.i3d_last_error(ctx.h).decode()),
                  (lambda dd, n, pp, s_, ft, ds, st: L.i3d_fusion_query_points(f.h, dd, n, pp, s_, None, ft, ds, None, st), lambda: L.i3d_fusion_last_error(f.h).decode()))
        for call, msg in models:
            cases = [((None, 4, p(pts), None, None, None, None), "descriptor"), ((d, 4, None, None, None, None, None), "points"),
                     ((d, -1, p(pts), None, None, None, None), "n must"), ((d, (1 << 27) + 1, p(pts), None, None, None, None), "n must"),
                     ((desc(max_steps=-1), 4, p(pts), None, None, None, None), "max_steps"), ((desc(max_steps=65), 4, p(pts), None, None, None, None), "max_steps"),
                     ((desc(tolerance_voxels=0.0), 4, p(pts), None, None, None, None), "tolerance"), ((desc(tolerance_voxels=-1e-6), 4, p(pts), None, None, None, None), "tolerance"),
                     ((desc(tolerance_voxels=float("nan")), 4, p(pts), None, None, None, None), "tolerance"),
                     ((desc(tolerance_voxels=float("inf")), 4, p(pts), None, None, None, None), "tolerance"),
                     ((desc(project=0), 4, p(pts), None, p(foot), None, None), "foot"), ((desc(project=0), 4, p(pts), None, None, p(dist), None), "distance")]
            for args, word in cases:
                assert call(*args) == 1 and word in msg(), (word, msg())
            st = B.QueryStats(); st.valid = 7; st.sum_abs_sdf = 3.0; st.steps = 9
            assert call(d, 0, None, None, None, None, C.byref(st)) == 0 and not any(st.as_dict().values())      # n = 0: success, zero stats
            assert call(desc(max_steps=64, project=0), 4, p(pts), p(sdf), None, None, C.byref(st)) == 0 and call(desc(max_steps=0), 4, p(pts), p(sdf), p(foot), p(dist), None) == 0
        with pytest.raises(ValueError):
            ctx.query_points(pts, outputs=("colour",))
        with pytest.raises(ValueError):
            f.query_points(pts, outputs=("albedo",))
        with pytest.raises(B.I3DError) as e:
            ctx.query_points(pts, outputs=("foot",), project=0)
        assert "failed (1)" in str(e.value) and "foot" in str(e.value)
    finally:
        f.close()
