"""-m gpu: i3d_fusion_register_volume on the device against its numpy statement (register_volume_twin.py): the selection bit for bit, the sums
within section 18.3's bound, the registration from three starts, the closed loop register -> merge, that the slot layout of src does not matter, that nothing else
moves, and the edges.

The selection runs on the merge tests' scenes (test_gpu_fusion_merge.scenes).  Those are a sphere with half-voxel bumps seen from one side: a rotation about its
centre is hardly observable there (the twin ends 3 degrees off on them), so the sums, the registration and the closed loop run on a scene of their own, `bumpy`:
the same sphere and cameras with bumps of 2 voxels at a wavelength of 16 voxels and no depth noise, volume A from frames 0-1 and volume B from frames 2-3 fused at
poses composed with T^-1, so that B's world is A's moved by a known T (x_A = T x_B).  The twin reaches status 0 on it from every start used here.

A volume's state is read with Fusion.debug_voxels over a dense box that holds all its stored voxels, as the merge tests do."""
import ctypes as C
import math

import numpy as np
import pytest

import fusion_cases as FC
import fusion_merge_twin as MT
import helpers
import query_twin as QT
import register_volume_twin as VT
import track_twin
from fusion_cases import fusion_frames, scenes  # noqa: F401  (fixtures)
from intrinsic3d_amd import binding as B, synthetic

pytestmark = pytest.mark.gpu

VS, VS2 = FC.VS, FC.VS2
FIELDS = ("found",) + FC.FIELDS
FACE_MARGIN = 1e-9                                  # voxels, as query_cases.FACE_MARGIN
ROT_FLOOR, TRANS_FLOOR = 1e-12, 1e-10               # section 18.3: rad, voxels
AXIS = np.array([0.3, -0.8, 0.52])


# ---- the scene of the sums, the registration and the closed loop ------------------------------------------------------------------------------------------------
def bumpy_frames():
    """(scene, A's frames, B's frames, T): four views of the bumpy sphere; B's frames carry poses composed with T^-1"""
    margin = int(np.ceil(FC.RADIUS_VOX + 3.2 + 4))
    scene = synthetic.Scene(np.full(3, (margin + 2) * VS), FC.RADIUS_VOX * VS, 2.0 * VS, 100.0)
    cam = track_twin.level_camera(FC.INTR, np.zeros(5), FC.W, FC.H, 0)
    intr = FC.INTR.astype(np.float32)
    R = synthetic.aa_to_rotmat(AXIS / np.linalg.norm(AXIS) * math.radians(6.0))
    t = scene.c - R @ scene.c + np.array([3.3, -2.1, 1.7]) * VS       # turns about the sphere's centre: B stays where A is, a few voxels off
    Tm = np.eye(4); Tm[:3, :3] = R; Tm[:3, 3] = t
    Tinv = np.linalg.inv(Tm)
    fa, fb = [], []
    for i in range(4):
        p = FC.orbit_pose(scene, 8.0 * i)
        d = track_twin.raycast_scene(scene, cam, track_twin.ref_from_pose(p))[0]
        c2w = helpers.c2w(p)
        fa.append((d, intr, FC.BGR, c2w, 2))
        fb.append((d, intr, FC.BGR, (Tinv @ c2w.astype(np.float64)).astype(np.float32), 2))
    return scene, fa, fb, VT.rt_to_pose(R, t)


def start_pose(scene, T, seed, deg=1.0, vox=1.5, centre=None):
    """T perturbed by a rotation of `deg` about the sphere's centre (or the one given) and a shift of `vox` voxels"""
    c = scene.c if centre is None else centre
    rng = np.random.default_rng(1); a = u = None
    for _ in range(seed + 1):
        a = rng.normal(size=3); a *= math.radians(deg) / np.linalg.norm(a)
        u = rng.normal(size=3); u *= vox * VS / np.linalg.norm(u)
    R, t = VT.pose_to_rt(T)
    dR = synthetic.aa_to_rotmat(a)
    return VT.rt_to_pose(dR @ R, dR @ (t - c) + c + u)


def _box_of(frames, vs):
    with FC.fuse(frames, vs) as f:
        f.finish(0); ex = f.export(); allocated = f.info()["allocated"]
    lo = ex["keys"].min(0).astype(np.int64) - 12; hi = ex["keys"].max(0).astype(np.int64) + 13
    box = FC.dense(lo, hi)
    with FC.fuse(frames, vs) as f:
        assert len(FC.snapshot(f, box)["keys"]) == allocated            # the box holds every stored voxel, the weightless ones included
    return box


class Bumpy:
    def __init__(self):
        self.scene, fa, fb, self.T = bumpy_frames()
        self.fa, self.fb, self.all_a = fa[:2], fb[2:], fa
        self.box_a, self.box_b = _box_of(fa, VS), _box_of(self.fb, VS)
        self.box_b2 = _box_of(self.fb, VS2)
        with self.a() as A, self.b() as Bv, self.b(vs=VS2) as B2:        # the reference: computed once, shared, left unchanged
            self.snap_a, self.snap_b, self.snap_b2 = FC.snapshot(A, self.box_a), FC.snapshot(Bv, self.box_b), FC.snapshot(B2, self.box_b2)
        self.grid = grid_of(self.snap_a, VS)

    def a(self):
        return FC.fuse(self.fa, VS)

    def b(self, capacity=1 << 16, vs=VS):
        return FC.fuse(self.fb, vs, capacity)


def grid_of(snap, vs):
    return QT.Grid(snap["keys"], snap["sdf"].astype(np.float64), snap["weight"], vs)


@pytest.fixture(scope="module")
def bumpy():
    return Bumpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_list(got, want):
    assert got["keys"].shape == want["keys"].shape, (got["keys"].shape, want["keys"].shape)
    assert np.array_equal(got["keys"].astype(np.int64), want["keys"]) and np.array_equal(_bits(got["sdf"]), _bits(want["sdf"]))


# ---- 1. the selection equals the twin exactly -----------------------------------------------------------------------------------------------------------------------
CASES = [(band, stride) for band in (1.0, 2.0) for stride in (1, 2, 3)]


def _check_selection(f, snap, vs, least=5):
    counts = []
    for band, stride in CASES:
        got = f.debug_register_volume_selection(source_band_voxels=band, stride=stride)
        _same_list(got, VT.select(snap, vs, band, stride))
        counts.append(len(got["sdf"]))
    assert min(counts) >= least and counts[3] > counts[0] > counts[1] > counts[2], counts
    return counts


def test_selection_equals_twin(scenes):
    s = scenes["overlapping"]
    with s.b() as Bv:
        counts = _check_selection(Bv, FC.snapshot(Bv, s.box), VS)
        print(f"selected at (band, stride) {CASES}: {counts}")
        # before and after finish(0): whatever finish leaves in the table is what the list is made of
        before = Bv.debug_register_volume_selection()
        Bv.finish(0)
        _check_selection(Bv, FC.snapshot(Bv, s.box), VS)
        assert len(Bv.debug_register_volume_selection()["sdf"]) <= len(before["sdf"])
    with B.Fusion(VS, 0.1, 10.0) as empty:
        assert len(empty.debug_register_volume_selection()["sdf"]) == 0


def test_selection_of_an_all_negative_volume(scenes):
    s = scenes["pow2"]; m = np.array((-70, -65, -80), np.int64)
    with B.Fusion(VS2, 0.1, 10.0, initial_capacity=1 << 16) as A, s.b() as Bv:
        A.merge(Bv, np.concatenate([np.zeros(3), m * VS2]))
        snap = FC.snapshot(A, FC.dense(s.lo + m, s.hi + m))
        assert (snap["keys"] < 0).all() and len(snap["keys"]) > 1000
        _check_selection(A, snap, VS2)
        got = A.debug_register_volume_selection(stride=3)
        assert (got["keys"] < 0).all() and (got["keys"] % 3 == 0).all() and len(got["sdf"]) >= 10


def test_selection_does_not_depend_on_the_table(scenes):
    s = scenes["overlapping"]
    with FC.fuse(s.frames, VS, 1 << 10) as small, FC.fuse(s.frames, VS, 1 << 16) as large:
        assert small.info()["capacity"] > 4096 and large.info()["capacity"] == 131072         # the first grew from 4 096 slots, the second never did
        for band, stride in CASES:
            a = small.debug_register_volume_selection(source_band_voxels=band, stride=stride)
            b = large.debug_register_volume_selection(source_band_voxels=band, stride=stride)
            assert len(a["sdf"]) >= 10 and np.array_equal(a["keys"], b["keys"]) and np.array_equal(_bits(a["sdf"]), _bits(b["sdf"]))
        _check_selection(small, FC.snapshot(small, s.box), VS)


# ---- 2. the sums equal the twin ---------------------------------------------------------------------------------------------------------------------------------------
def _check_sums(dev, valid, selected, tw, sel, vs_f, gate):
    n = tw["n"]
    assert selected == len(sel["keys"]) and valid == tw["valid"] and int(dev[28]) == tw["inliers"], (selected, valid, tw["valid"], dev[28], tw["inliers"])
    assert tw["face_margin"] >= FACE_MARGIN and tw["gate_margin"] >= FACE_MARGIN * vs_f, (tw["face_margin"], tw["gate_margin"])     # a condition on the inputs
    err = np.abs(dev - tw["sums"]); tol = n * 2.0 ** -52 * tw["abs_sums"]
    print(f"  n = {n}: valid {valid}, inliers {tw['inliers']}, worst error / bound {np.max(err / np.maximum(tol, 1e-300)):.3f}, gate {gate:.3e}")
    assert np.all(err <= tol), (err, tol)


def _sums_case(A, Bv, grid, snap_b, vs_b, pose, gate, limits, row_cap=0, band=2.0):
    sel = VT.select(snap_b, vs_b, band, 1)
    c = VT.pivot(grid, sel, pose) + np.array([0.3, -0.2, 0.1]) * VS        # a given pivot, not the call's own
    R, t = VT.pose_to_rt(pose)
    out = []
    for limit in limits:
        dev, valid, selected = A.debug_register_volume_sums(Bv, pose, c, limit=limit, row_cap=row_cap, max_distance=gate, source_band_voxels=band)
        tw = VT.sums(grid, sel, R, t - c, c, gate, limit=limit)
        _check_sums(dev, valid, selected, tw, sel, grid.vs, gate)
        out.append((dev, valid, tw))
    return out, sel, c


def _quarter_gate(grid, snap_b, vs_b, pose):
    """a gate between two neighbouring |r| at the lower quartile of the valid samples"""
    sel = VT.select(snap_b, vs_b, 2.0, 1)
    c = VT.pivot(grid, sel, pose) + np.array([0.3, -0.2, 0.1]) * VS
    R, t = VT.pose_to_rt(pose)
    tw = VT.sums(grid, sel, R, t - c, c, 0.05)
    r = np.sort(np.abs(tw["r"][tw["valid_mask"]]))
    k = len(r) // 4
    while r[k + 1] - r[k] < 1e-6 * VS:
        k += 1
    return 0.5 * (r[k] + r[k + 1])


def test_sums_equal_twin(bumpy):
    pose = start_pose(bumpy.scene, bumpy.T, 0)
    with bumpy.a() as A, bumpy.b() as Bv:
        print("all inliers:")
        runs, sel, c = _sums_case(A, Bv, bumpy.grid, bumpy.snap_b, VS, pose, 0.05, (1, 63, 65, 257, 449, 513, 0))
        full = runs[-1]
        assert full[2]["n"] == len(sel["keys"]) > 1000 and full[2]["inliers"] == full[2]["valid"] > 500
        assert [r[2]["n"] for r in runs[:6]] == [1, 63, 65, 257, 449, 513] and runs[3][2]["valid"] > 0
        # B's first entries in key order lie at the rim A does not see; against a second copy of B itself, a little moved, the short lists are valid too
        print("against its own copy:")
        Rt, tt = VT.pose_to_rt(bumpy.T)
        near = start_pose(bumpy.scene, np.zeros(6), 2, deg=0.7, vox=0.8, centre=Rt.T @ (bumpy.scene.c - tt))
        with bumpy.b() as copy:
            own = _sums_case(copy, Bv, grid_of(bumpy.snap_b, VS), bumpy.snap_b, VS, near, 0.05, (1, 63, 65, 257, 0))[0]
        assert own[1][1] > 0 and own[2][1] > 0 and own[3][1] > 32 and own[4][1] > 500
        print("a quarter of the inliers:")
        gate = _quarter_gate(bumpy.grid, bumpy.snap_b, VS, pose)
        cut = _sums_case(A, Bv, bumpy.grid, bumpy.snap_b, VS, pose, gate, (65, 0))[0][-1]
        assert 0.2 * cut[2]["valid"] < cut[2]["inliers"] < 0.3 * cut[2]["valid"]
        print("row_cap = 8, the whole stored band: every lane walks at least two entries")
        wide = _sums_case(A, Bv, bumpy.grid, bumpy.snap_b, VS, pose, 0.05, (0,), row_cap=8, band=5.5)[0][-1]
        assert wide[2]["n"] > 8 * 256                                      # P >= 2
        free = _sums_case(A, Bv, bumpy.grid, bumpy.snap_b, VS, pose, 0.05, (0,), band=5.5)[0][-1]
        assert wide[1] == free[1] and wide[0][28] == free[0][28]           # the same counts at P = 1
        # two identical calls are bit-identical
        again = A.debug_register_volume_sums(Bv, pose, c, max_distance=0.05)
        assert np.array_equal(again[0], full[0]) and again[1] == full[1]


def test_sums_with_different_voxel_sizes(bumpy):
    pose = start_pose(bumpy.scene, bumpy.T, 1)
    with bumpy.a() as A, bumpy.b(vs=VS2) as B2:
        runs, sel, _ = _sums_case(A, B2, bumpy.grid, bumpy.snap_b2, VS2, pose, 0.05, (65, 0))
        assert runs[-1][2]["valid"] > 500 and len(sel["keys"]) > 1000
        assert np.array_equal(sel["points"], sel["keys"].astype(np.float64) * VS2)      # metric points on src's own lattice


# ---- 3. the registration equals the twin ---------------------------------------------------------------------------------------------------------------------------
COUNTS = ("status", "iterations", "selected", "valid", "inliers")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_registration_equals_twin(bumpy, seed):
    start = start_pose(bumpy.scene, bumpy.T, seed)
    tw, ts = VT.register(bumpy.grid, bumpy.snap_b, VS, start)
    sq, ss = VT.register(bumpy.grid, bumpy.snap_b, VS, start, order="sequential")
    own = VT.pose_diff(tw, sq, VS)                                        # what the order of the sums alone does to the result, measured without the device
    bar = max(10.0 * own[0], ROT_FLOOR), max(10.0 * own[1], TRANS_FLOOR)
    assert ts["face_margin"] >= FACE_MARGIN and ts["gate_margin"] >= FACE_MARGIN * VS
    assert (ts["status"], ts["iterations"]) == (ss["status"], ss["iterations"]) and ts["status"] == 0
    with bumpy.a() as A, bumpy.b() as Bv:
        pose, st = A.register_volume(Bv, start)
    ang, tr = VT.pose_diff(pose, tw, VS)
    print(f"start {seed}: status {st['status']} after {st['iterations']} steps, {st['selected']} selected / {st['valid']} valid / {st['inliers']} inliers; device against "
          f"twin {ang:.3e} rad, {tr:.3e} voxel; the twin's two orders {own[0]:.3e} rad, {own[1]:.3e} voxel; bar {bar[0]:.1e} rad, {bar[1]:.1e} voxel")
    assert {k: st[k] for k in COUNTS} == {k: ts[k] for k in COUNTS}, (st, ts)
    assert ang <= bar[0] and tr <= bar[1]
    for k in ("rms_initial", "rms_final", "min_pivot_ratio"):
        assert abs(st[k] - ts[k]) <= 1e-9 * abs(ts[k]), (k, st[k], ts[k])


# ---- 4. the loop closes -------------------------------------------------------------------------------------------------------------------------------------------------
def _surface_points(scene):
    """points on the ground-truth surface of the side the cameras see"""
    rng = np.random.default_rng(4)
    look = np.array([math.sin(math.radians(12.0)), math.sin(math.radians(20.0)), math.cos(math.radians(12.0))])
    dirs = rng.normal(size=(6000, 3)) * 0.5 + look; dirs /= np.sqrt((dirs * dirs).sum(1, keepdims=True))
    dirs = dirs[dirs @ look > 0.8][:2000]
    p = scene.c + dirs * scene.R
    for _ in range(30):                                                   # along the radius, damped: the bumps make the field's slope differ from 1
        d = p - scene.c
        p = p - 0.7 * scene.sdf(p)[:, None] * d / np.sqrt((d * d).sum(1, keepdims=True))
    assert np.abs(scene.sdf(p)).max() < 1e-9
    return p


# Band: the two volumes are projective TSDFs of different views, so their values agree at the surface and drift apart away from it.  On these volumes the twin ends
# 0.94 degrees / 0.74 voxel off T with the default band of 2 voxels and 0.25 degrees / 0.15 voxel with 1 voxel; the loop is closed with the narrower band.
LOOP = dict(source_band_voxels=1.0)


def test_the_loop_closes(bumpy):
    T = bumpy.T
    start = start_pose(bumpy.scene, T, 2)
    tw, ts = VT.register(bumpy.grid, bumpy.snap_b, VS, start, LOOP)
    assert ts["status"] == 0                                              # the twin converges on this scene within the default budget
    own = VT.pose_diff(tw, T, VS)                                         # the method's own error on these two volumes, measured without the device
    bar = 2.5 * own[0], 2.5 * own[1]                                      # section 18.3's margin of the device over the twin
    pts = _surface_points(bumpy.scene)
    mean = {}
    with bumpy.a() as A, bumpy.b() as Bv:
        pose, st = A.register_volume(Bv, start, **LOOP)
        got = VT.pose_diff(pose, T, VS)
        for name, p in (("found", pose), ("start", start), ("T", T)):
            with bumpy.a() as M:
                M.merge(Bv, p)
                q = M.query_points(pts, project=0)["stats"]
                assert q["valid"] > 1000
                mean[name] = q["sum_abs_sdf"] / q["valid"]
        own_a = A.query_points(pts, project=0)["stats"]
    s0 = VT.pose_diff(start, T, VS)
    print(f"start {math.degrees(s0[0]):.3f} deg / {s0[1]:.3f} voxel off T; device {math.degrees(got[0]):.4f} deg / {got[1]:.4f} voxel off T after {st['iterations']} steps "
          f"(status {st['status']}); twin {math.degrees(own[0]):.4f} deg / {own[1]:.4f} voxel; bar {math.degrees(bar[0]):.4f} deg / {bar[1]:.4f} voxel")
    print(f"mean |sdf| at the ground-truth surface after the merge: under the pose found {mean['found']:.4e} m, under the start {mean['start']:.4e} m, under T "
          f"{mean['T']:.4e} m; A alone {own_a['sum_abs_sdf'] / own_a['valid']:.4e} m")
    assert st["status"] == 0 and got[0] <= bar[0] and got[1] <= bar[1]
    assert mean["found"] <= mean["start"]


# ---- 5. the slot layout of src does not matter -------------------------------------------------------------------------------------------------------------------------
def test_slot_layout_does_not_matter(bumpy):
    start = start_pose(bumpy.scene, bumpy.T, 1)
    with bumpy.a() as A, bumpy.b(1 << 10) as small, bumpy.b(1 << 16) as large:
        assert small.info()["capacity"] > 4096 and large.info()["capacity"] == 131072
        p0, s0 = A.register_volume(small, start)
        p1, s1 = A.register_volume(large, start)
        p2, s2 = A.register_volume(small, start)
    assert s0["iterations"] > 0 and np.array_equal(p0, p1) and s0 == s1 and np.array_equal(p0, p2) and s0 == s2


# ---- 6. nothing else moves ------------------------------------------------------------------------------------------------------------------------------------------------
def _state(f, box):
    dv = f.debug_voxels(box)
    return dv, f.info()


def _same_state(a, b):
    for k in FIELDS:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert a[1] == b[1]


def test_nothing_else_moves(bumpy):
    start = start_pose(bumpy.scene, bumpy.T, 0)
    fr = bumpy.all_a
    h, w = fr[0][0].shape
    args = lambda i: (fr[i][0], fr[i][1], fr[i][2], fr[i][1], fr[i][3], fr[i][4])  # noqa: E731
    cam = dict(width=w, height=h, intr=FC.INTR, pose=FC.orbit_pose(bumpy.scene, 8.0))
    with bumpy.a() as A, bumpy.a() as never, bumpy.b() as Bv, bumpy.b() as fresh:
        a0, b0 = _state(A, bumpy.box_a), _state(Bv, bumpy.box_b)
        r0 = A.render(cam)                                                # builds A's cached brick bitmap
        assert r0["stats"]["hits"] > 500
        pose, st = A.register_volume(Bv, start)
        assert st["iterations"] > 0 and st["status"] == 0
        _same_state(_state(A, bumpy.box_a), a0); _same_state(_state(Bv, bumpy.box_b), b0)
        assert A.info()["frames"] == 2 and Bv.info()["frames"] == 2       # no ordinal consumed
        FC.same_render(A.render(cam), r0); FC.same_render(never.render(cam), r0)
        # integrate, deintegrate and merge behave as on a volume never registered (nor registered from)
        box = np.concatenate([bumpy.box_a, bumpy.box_b])
        assert A.integrate(*args(2)) == never.integrate(*args(2)) == 2
        _same_state(_state(A, box), _state(never, box))
        A.deintegrate(0, *args(0)); never.deintegrate(0, *args(0))
        _same_state(_state(A, box), _state(never, box))
        m0, m1 = A.merge(Bv, pose), never.merge(fresh, pose)
        assert {k: m0[k] for k in FC.COUNTS} == {k: m1[k] for k in FC.COUNTS} and m0["allocated"] > 0
        big = FC.dense(box.min(0) - 6, box.max(0) + 7)
        _same_state(_state(A, big), _state(never, big))
        ea, eb = A.export(), never.export()
        ex, ef = Bv.export(), fresh.export()                              # finish after having been registered from
        for k in ("keys", "sdf", "weight", "color"):
            assert np.array_equal(ea[k], eb[k]) and np.array_equal(ex[k], ef[k]), k
        # finished volumes are read as they stand
        p2, s2 = A.register_volume(Bv, start)
        assert s2["selected"] > 500 and s2["valid"] > 500


# ---- 7. edges -------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_edges(bumpy):
    start = start_pose(bumpy.scene, bumpy.T, 0)
    with bumpy.a() as A, bumpy.b() as Bv, B.Fusion(VS, 0.1, 10.0) as empty:
        for f, src, desc, selected in ((A, empty, {}, 0), (A, Bv, dict(source_band_voxels=1e-9), 0), (empty, Bv, {}, None)):
            pose, st = f.register_volume(src, start, **desc)
            assert st["status"] == 2 and st["iterations"] == 0 and np.array_equal(pose, start), st
            assert st["selected"] == selected if selected is not None else st["selected"] > 500 and st["valid"] == 0
        pose, st = A.register_volume(Bv, start, iterations=0)              # figures only
        assert np.array_equal(pose, start) and (st["status"], st["iterations"]) == (1, 0) and st["inliers"] > 500 and st["rms_initial"] == st["rms_final"] > 0
        pose, s1 = A.register_volume(Bv, start, iterations=1)
        assert (s1["status"], s1["iterations"]) == (1, 1) and not np.array_equal(pose, start) and abs(s1["rms_initial"] - st["rms_final"]) <= 1e-12 * st["rms_final"] and s1["rms_final"] < st["rms_final"]

        L = B.load(); p = B._p
        stats = B.RegisterVolumeStats(); stats.selected = 77
        good = B.register_volume_desc_default()
        po = start.copy()

        def refused(call, word, f=A):
            assert call() == 1 and word in L.i3d_fusion_last_error(f.h).decode(), L.i3d_fusion_last_error(f.h).decode()
            assert np.array_equal(po, start) and stats.selected == 77

        assert L.i3d_fusion_register_volume(None, Bv.h, C.byref(good), p(po), C.byref(stats)) == 1
        refused(lambda: L.i3d_fusion_register_volume(A.h, None, C.byref(good), p(po), C.byref(stats)), "null source")
        refused(lambda: L.i3d_fusion_register_volume(A.h, Bv.h, None, p(po), C.byref(stats)), "null descriptor")
        refused(lambda: L.i3d_fusion_register_volume(A.h, Bv.h, C.byref(good), None, C.byref(stats)), "null pose")
        refused(lambda: L.i3d_fusion_register_volume(A.h, A.h, C.byref(good), p(po), C.byref(stats)), "to itself")
        for field, values, word in (("iterations", (-1, 201), "iterations"), ("stride", (0, 65, -2), "stride"),
                                    ("source_band_voxels", (0.0, -1.0, math.nan, math.inf), "source_band_voxels"), ("max_distance", (0.0, math.nan, math.inf), "max_distance")):
            for v in values:
                d = B.register_volume_desc_default(**{field: v})
                refused(lambda: L.i3d_fusion_register_volume(A.h, Bv.h, C.byref(d), p(po), C.byref(stats)), word)
        for k, v in ((0, math.nan), (4, math.inf)):
            bad = start.copy(); bad[k] = v; keep = bad.copy()
            assert L.i3d_fusion_register_volume(A.h, Bv.h, C.byref(good), p(bad), C.byref(stats)) == 1 and "not finite" in L.i3d_fusion_last_error(A.h).decode()
            assert np.array_equal(bad, keep, equal_nan=True) and stats.selected == 77
        try:
            far = B.Fusion(VS, 0.1, 10.0, device=1)                        # only where the machine has a second device
        except B.I3DError:
            far = None
        if far is not None:
            with far:
                refused(lambda: L.i3d_fusion_register_volume(A.h, far.h, C.byref(good), p(po), C.byref(stats)), "different devices")
        with pytest.raises(ValueError):
            A.register_volume(None, start)
        pose, st = A.register_volume(Bv, start)                            # the handle goes on working
        assert st["status"] == 0
