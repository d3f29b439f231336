"""-m "not gpu": the numpy statement of i3d_query_points (query_twin.py) against the analytic sphere, the input condition of the point sets the device is compared
on (query_cases.py), and the agreement of the query twin with the render twin that sets the device's bar."""

import numpy as np

import query_cases as Q
import query_twin as T
import render_twin

# Measured here with the twin on the sphere of radius 12 voxels, exact fp64 distances in a band of 3.2 voxels, 4000 points within 2 voxels of the surface, and
# written into DESIGN.md 17.1 (voxels): trilinear value against |p - c| - R 0.0245 (the interpolation error h^2 / (4 r) of a distance field at r >= 10 voxels is
# 0.025); feet off the sphere 0.0209; signed distance against |p - c| - R 0.0215.  The bars are those figures rounded up.
SDF_BAR_VOX, FOOT_BAR_VOX, DISTANCE_BAR_VOX = 0.03, 0.025, 0.025
# the query twin on the render twin's hits of query_cases.view_camera (depth cast to fp32): max |sdf| 9.4e-4 voxel, max angle 1.4e-7 rad; the device's bars are
# 10 x what the twins give at run time (test_gpu_query.py), these only pin the order of magnitude quoted in DESIGN.md 17.3
VIEW_SDF_VOX, VIEW_ANGLE = 2e-3, 5e-7


def test_twin_against_the_analytic_sphere():
    g = Q.sphere_grid(bump_amp_vox=0.0, hole=False)
    grid = Q.twin_grid(g, refined=False)
    pts = Q._band_points(g, np.random.default_rng(5), 4000, spread_vox=2.0, avoid_cap=False)
    tw = T.query(grid, pts)
    c, R = g["scene"].c, g["scene"].R
    ana = np.sqrt(((pts - c) ** 2).sum(1)) - R
    b0, b1 = (tw["status"] & 1) != 0, (tw["status"] & 2) != 0
    assert b0.sum() > 3900 and b1.sum() > 3900 and not (b1 & ~b0).any()
    e_sdf = np.abs(tw["sdf"] - ana)[b0].max() / Q.VS
    e_foot = np.abs(np.sqrt(((tw["foot"] - c) ** 2).sum(1)) - R)[b1].max() / Q.VS
    e_dist = np.abs(tw["distance"] - ana)[b1].max() / Q.VS
    radial = c + (pts - c) * (R / np.sqrt(((pts - c) ** 2).sum(1)))[:, None]
    e_closest = np.sqrt(((tw["foot"] - radial) ** 2).sum(1))[b1].max() / Q.VS
    print(f"sdf {e_sdf:.4f} foot {e_foot:.4f} distance {e_dist:.4f} voxel; foot against the exact closest point {e_closest:.4f} voxel; "
          f"steps mean {tw['steps'][b1].mean():.2f} max {tw['steps'].max()}")
    assert e_sdf <= SDF_BAR_VOX and e_foot <= FOOT_BAR_VOX and e_dist <= DISTANCE_BAR_VOX
    assert e_closest <= 0.2                                       # the foot of the gradient path is not the closest point (17.1 quotes 0.105)
    assert np.all(np.sign(tw["distance"][b1]) == np.sign(tw["sdf"][b1]))
    nrm = (pts - c) / np.sqrt(((pts - c) ** 2).sum(1, keepdims=True))
    # the gradient of the trilinear interpolant is off by up to h / 2 times the second derivative 1 / r per axis: sqrt(3) * 0.5 / 10 rad = 5 degrees at r >= 10 voxels
    assert np.degrees(np.arccos(np.clip((tw["normal"] * nrm).sum(1), -1, 1)))[b0].max() < 5.0
    for k in ("foot", "distance"):
        assert not tw[k][~b1].any()
    assert not tw["sdf"][~b0].any() and not tw["normal"][~b0].any()
    # converged means |f| <= tolerance at the foot, and a foot queried again takes no step
    again = T.query(grid, tw["foot"][b1])
    assert np.all(again["status"] == 3) and not again["steps"].any() and not again["distance"].any() and np.array_equal(again["foot"], tw["foot"][b1])
    assert np.abs(again["sdf"]).max() <= 1e-6 * Q.VS
    none = T.query(grid, pts, max_steps=0)
    assert not none["steps"].any() and ((none["status"] & 2) != 0).sum() < 5


def test_checked_point_sets_meet_the_input_condition():
    for i in range(len(Q.PROJECTION_SETS)):
        g, refined, pts, tw = Q.projection_set(i)
        assert pts.shape == (Q.PROJECTION_SETS[i][1], 3)
        again = T.query(Q.twin_grid(g, refined), pts, trace=True)            # the set as the device test will see it
        assert np.all(again["status"] == 3), i
        assert T.all_valid(again["trace"]).all(), i
        assert T.face_margin(again["trace"]).min() >= Q.FACE_MARGIN, i
        assert again["steps"].max() <= 8 and again["steps"].min() >= 1
    g = Q.plain()
    cap = Q.cap_points(g, 100, 21)
    tw = T.query(Q.twin_grid(g), cap, trace=True)
    assert cap.shape == (100, 3) and np.all(tw["status"] == 1) and T.face_margin(tw["trace"]).min() >= Q.FACE_MARGIN
    assert not T.all_valid(tw["trace"]).any() and tw["steps"].min() >= 1


def test_value_set_covers_its_cases():
    g = Q.plain()
    tw = T.query(Q.twin_grid(g), Q.value_points(g, 31), project=False)
    st = tw["status"]
    assert set(np.unique(st)) == {0, 1} and (st == 1).sum() > 2500 and (st == 0).sum() > 400
    assert not st[-9:-2].any()                                    # NaN, inf, 1e30, 1e300, |q| >= 2^20: invalid without a lookup
    around = st[-9 - 64:-9].reshape(4, 4, 4)                      # the cells around the voxel of weight 0: exactly the 8 that touch it are invalid
    assert not around[1:3, 1:3, 1:3].any() and around.sum() == 64 - 8
    gn = Q.negative()
    tn = T.query(Q.twin_grid(gn), Q.value_points(gn, 32), project=False)
    assert tn["status"][-2] == 1 and tn["status"][-1] == 1        # q = -0.5: the cell based at -1
    gs = Q.shifted()
    assert np.abs(gs["keys"]).min() > 99000
    # the voxel centres really have fraction 0 in the kernel's q = p / vs, and the points just below an integer land in the cell one lower, a fraction
    # within 1e-9 of 1, on every grid
    seg = Q.value_segments()
    for gg, seed in ((g, 31), (gn, 32), (gs, 31)):
        pts = Q.value_points(gg, seed)
        assert pts.shape[0] == seg["special"].stop
        q = pts[seg["centres"]] / Q.VS
        assert np.array_equal(q, np.round(q)) and ((q - np.floor(q)) == 0.0).all()
        tc = T.query(Q.twin_grid(gg), pts[seg["centres"]], project=False)
        assert (tc["status"] == 1).sum() > 100                     # many of them in valid cells
        qb = pts[seg["below"]] / Q.VS
        k = np.round(pts[seg["centres"]][:100] / Q.VS)
        lower = np.floor(qb[:, 0]) == k[:, 0] - 1
        assert lower.sum() >= 90 and ((qb[:, 0] - np.floor(qb[:, 0]))[lower] > 1.0 - 1e-9).all()


def test_query_twin_agrees_with_render_twin():
    g = Q.plain()
    grid = Q.twin_grid(g)
    cam = Q.view_camera(g)
    rt = render_twin.render(grid, render_twin.camera_from_pose(cam["pose"], cam["intr"], cam["dist"], cam["width"], cam["height"]))
    assert rt["hit"].sum() > 250
    pts, (hv, hu) = Q.view_points(cam, rt["depth"].astype(np.float32), rt["dir"])
    tq = T.query(grid, pts, project=False)
    assert np.all(tq["status"] == 1)
    e_sdf = np.abs(tq["sdf"]).max() / Q.VS
    ang = Q.angle(rt["normal"][hv, hu].astype(np.float32), tq["normal"]).max()
    print(f"view: max |sdf| {e_sdf:.3e} voxel, max angle {ang:.3e} rad over {hv.size} hits")
    assert e_sdf <= VIEW_SDF_VOX and ang <= VIEW_ANGLE
