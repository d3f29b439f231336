"""-m gpu: i3d_fusion_prune on the device against its numpy statement (fusion_prune_twin.py), bit for bit over every stored voxel: each
criterion alone and together, the defaults under every reader of the model, a call that removes nothing, the crank rule, frames taken out and moved after a prune,
the rebuilt table (shrink, growth, repeatability), the lane and workgroup edges, a pruned volume as the source of a general merge, the errors, and app_fusion.

The state of a volume is read with Fusion.debug_voxels over ONE dense box of keys that holds every stored voxel, the weight-0 ones included (fusion_cases.Scene
asserts it), so two states over the box compare element by element.  Every threshold comes from the volume's own state, so each criterion splits it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fusion_cases as FC
import fusion_deintegrate_twin as DT
import fusion_load_twin as LT
import fusion_merge_twin as MT
import fusion_prune_twin as PT
from fusion_cases import fusion_frames, scenes  # noqa: F401  (fixtures)
from intrinsic3d_amd import binding as B, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

F = np.float32
FIELDS = ("sdf", "weight", "color")
STATE = ("found",) + FIELDS + ("first_frame",)
RECORD = ("keys", "sdf", "weight", "color")
COUNTS = ("stored", "removed", "failed_weight", "failed_sdf", "failed_box")
OK, INVALID, ERR_STATE = 0, 1, 4
OFF = dict(min_weight=-1.0)                          # W off; S and B are off by default


def _args(fr):
    d, intr, bgr, T, er = fr
    return d, intr, bgr, intr, T, er


def _fuse(s, n, capacity=1 << 16, first=0):
    f = B.Fusion(s.vs, 0.1, 10.0, initial_capacity=capacity)
    for fr in s.frames[first:first + n]:
        f.integrate(*_args(fr))
    return f


def _state(f, box):
    return f.debug_voxels(box)


def _same_state(a, b, fields=STATE):
    for k in fields:
        assert np.array_equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))


def _same_records(a, b):
    assert len(a["sdf"]) == len(b["sdf"]), (len(a["sdf"]), len(b["sdf"]))
    for k in RECORD:
        assert np.array_equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))


def _volume(st, box):
    s = st["found"]
    return MT.volume(box[s], st["sdf"][s], st["weight"][s], st["color"][s], st["first_frame"][s])


def _by_key(vol):
    return LT.volume_of(vol["keys"], vol["sdf"], vol["weight"], vol["color"], vol["first_frame"])


def _masked(st, found):
    """a state over the box with everything outside `found` as debug_voxels reports a key that is not stored"""
    out = dict(found=found.copy(), sdf=np.where(found, st["sdf"], F(0)), weight=np.where(found, st["weight"], F(0)),
               color=np.where(found[:, None], st["color"], np.uint8(0)))
    if "first_frame" in st:
        out["first_frame"] = np.where(found, st["first_frame"], -1)
    return out


def _pruned_state(st, keys, vs, **params):
    """the twin's verdict applied to a state over the box of keys: (state, removed mask over the box)"""
    v = np.zeros(len(keys), np.uint8); s = st["found"]
    v[s] = PT.verdict(keys[s], st["sdf"][s], st["weight"][s], vs, **params)
    return _masked(st, s & (v == 0)), v != 0


def _thresholds(st, box, s):
    """from the volume's own state: the median of the positive weights, the median |sdf| of the weighted voxels, a box whose x1 face goes through the key centroid"""
    on = st["found"]; w = st["weight"][on]; sd = st["sdf"][on]
    wmed = float(F(np.median(w[w > 0]))); smed = float(F(np.median(np.abs(sd[w > 0]))))
    cx = float(box[on][:, 0].astype(np.float64).mean()) * s.vs
    half = np.array([(s.lo[0] - 1) * s.vs, cx, (s.lo[1] - 1) * s.vs, (s.hi[1] + 1) * s.vs, (s.lo[2] - 1) * s.vs, (s.hi[2] + 1) * s.vs], F)
    return wmed, smed, half


def _cases(wmed, smed, half):
    return dict(weight=dict(min_weight=wmed), sdf=dict(min_weight=-1.0, max_abs_sdf=smed), box=dict(min_weight=-1.0, box=half),
                all=dict(min_weight=wmed, max_abs_sdf=smed, box=half), erase=dict(min_weight=-1.0, box=half, box_mode=2))


def _counts(c):
    return [c[k] for k in COUNTS]


def _stored_inside(f, st):
    order = f.debug_insertion_order()
    assert len(order) == int(st["found"].sum()), ("stored", len(order), "inside the box", int(st["found"].sum()))
    return order


# ---- 1. each criterion alone, all three, and mode 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["weight", "sdf", "box", "all", "erase"])
@pytest.mark.parametrize("name", ["textured", "overlapping"])
def test_criteria_equal_the_twin(scenes, name, case):
    s = scenes[name]
    with _fuse(s, len(s.frames)) as f:
        st0 = _state(f, s.box); order0 = _stored_inside(f, st0); info0 = f.info()
        params = _cases(*_thresholds(st0, s.box, s))[case]
        counts = f.prune(**params)
        st1 = _state(f, s.box); order1 = _stored_inside(f, st1); info1 = f.info()
        n = f.snapshot(); snap = f.export()
    want, want_order, want_counts = PT.prune(_volume(st0, s.box), order0, voxel_size=s.vs, **params)
    print(f"{name} / {case}: stored {counts['stored']}, removed {counts['removed']} (W {counts['failed_weight']}, S {counts['failed_sdf']}, B {counts['failed_box']})")
    assert _counts(counts) == want_counts
    assert 0 < counts["removed"] < counts["stored"] == len(order0)
    got = _volume(st1, s.box)
    for k in ("keys",) + FIELDS + ("first_frame",):
        assert np.array_equal(got[k], want[k]), (k, len(got[k]), len(want[k]))
    assert np.array_equal(order1, want_order)
    assert info1 == info0                                                   # no ordinal consumed, the capacity kept (shrink = 0)
    rec = LT.snapshot_records(_by_key(want), want_order)
    assert n == len(rec["sdf"])
    _same_records(snap, rec)
    if case == "all":                                                       # a voxel failing several criteria counts in each
        assert counts["failed_weight"] + counts["failed_sdf"] + counts["failed_box"] > counts["removed"]
    if case in ("box", "erase"):
        assert counts["failed_box"] == counts["removed"] and counts["failed_weight"] == counts["failed_sdf"] == 0


def test_mode_2_removes_what_mode_1_keeps(scenes):
    s = scenes["textured"]
    with _fuse(s, 3) as f, _fuse(s, 3) as g:
        st0 = _state(f, s.box)
        _, _, half = _thresholds(st0, s.box, s)
        a = f.prune(min_weight=-1.0, box=half); b = g.prune(min_weight=-1.0, box=half, box_mode=2)
        sa, sb = _state(f, s.box), _state(g, s.box)
    assert a["removed"] + b["removed"] == a["stored"] == b["stored"]
    assert np.array_equal(sa["found"] ^ sb["found"], st0["found"]) and not (sa["found"] & sb["found"]).any()


# ---- 2. the defaults: exactly the weightless voxels, and no reader of the model sees a difference -----------------------------------------------------------------
def _camera(s, i):
    d, intr, _, T, _ = s.frames[i]
    return dict(width=d.shape[1], height=d.shape[0], intr=np.asarray(intr, np.float64), pose=B.pose_mat_to_vec6(T))


def _camera_rays(cam):
    p = cam["pose"]; R = synthetic.aa_to_rotmat(p[:3]); fx, fy, cx, cy = [float(x) for x in cam["intr"]]
    v, u = np.mgrid[0:cam["height"], 0:cam["width"]]
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, np.float64)], -1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(-R.T @ p[3:], (len(d), 1)), d @ R


def _readers(f, s, pts):
    cam = _camera(s, 1)
    o, d = _camera_rays(cam)
    start = _camera(s, 2)["pose"] + np.array([0.004, -0.003, 0.002, 0.003, -0.002, 0.004])
    return dict(render=f.render(cam), rays=f.cast_rays(o, d), query=f.query_points(pts), mesh=f.extract_mesh(),
                track=f.track_sdf(s.frames[2][0], start, cam["intr"]))


@pytest.mark.parametrize("name", ["textured", "overlapping"])
def test_defaults_remove_the_weightless_and_no_reader_notices(scenes, name):
    s = scenes[name]
    with _fuse(s, 3) as f, _fuse(s, 3) as plain:
        st0 = _state(f, s.box)
        on = st0["found"] & (st0["weight"] > 0)
        rng = np.random.default_rng(11)
        sel = rng.choice(int(on.sum()), 2000, replace=False)
        pts = (s.box[on][sel] + rng.uniform(-0.5, 0.5, (2000, 3))) * s.vs
        before = _readers(f, s, pts)
        counts = f.prune()
        after = _readers(f, s, pts)
        st1 = _state(f, s.box)
        nf = f.finish(0); rf = f.export()
        npl = plain.finish(0); rp = plain.export()
    weightless = st0["found"] & ~(st0["weight"] > 0)
    print(f"{name}: stored {counts['stored']}, weightless removed {counts['removed']}")
    assert counts["removed"] == counts["failed_weight"] == int(weightless.sum()) > 0 and counts["failed_sdf"] == counts["failed_box"] == 0
    _same_state(st1, _masked(st0, on))
    a, b = before["render"], after["render"]
    assert a["stats"] == b["stats"] and a["stats"]["hits"] > 100
    for k in ("depth", "normal"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    a, b = before["rays"], after["rays"]
    assert a["stats"] == b["stats"] and a["stats"]["hits"] > 100
    for k in ("t", "position", "normal", "status"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    a, b = before["query"], after["query"]
    assert a["stats"] == b["stats"] and np.isfinite(a["sdf"]).sum() > 100
    for k in ("sdf", "normal", "status"):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    a, b = before["mesh"], after["mesh"]
    assert len(a[0]) > 100 and len(a[2]) > 100
    for x, y, what in zip(a, b, ("vertices", "colors", "faces")):
        assert np.array_equal(x, y), what
    (pa, sa), (pb, sb) = before["track"], after["track"]
    assert np.array_equal(pa, pb) and sa == sb and sa["valid"] > 100
    # the finish(0) records as a SET, by key: those of a volume never pruned (their order may differ, section 38.1 item 8)
    assert nf == npl == int(on.sum())
    ia, ib = np.argsort(LT.pack(rf["keys"])), np.argsort(LT.pack(rp["keys"]))
    for k in RECORD:
        assert np.array_equal(rf[k][ia], rp[k][ib]), k


# ---- 3. nothing removed: the table is not touched ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shrink", [False, True])
def test_nothing_removed_leaves_the_table_alone(scenes, shrink):
    s = scenes["textured"]
    with _fuse(s, 2) as f, _fuse(s, 2) as plain:
        st0 = _state(f, s.box); order0 = _stored_inside(f, st0); info0 = f.info()
        counts = f.prune(shrink=shrink, **OFF)
        assert _counts(counts) == [len(order0), 0, 0, 0, 0] and len(order0) > 1000
        assert PT.capacity_after(info0["capacity"], len(order0), 1, True) < info0["capacity"]          # a shrink that acted would show
        _same_state(_state(f, s.box), st0)
        assert np.array_equal(f.debug_insertion_order(), order0) and f.info() == info0
        assert f.integrate(*_args(s.frames[2])) == plain.integrate(*_args(s.frames[2])) == 2
        _same_state(_state(f, s.box), _state(plain, s.box))
        assert np.array_equal(f.debug_insertion_order(), plain.debug_insertion_order())
        assert f.finish(10) == plain.finish(10) > 1000
        _same_records(f.export(), plain.export())


# ---- 4. the crank rule: a later frame expands the blocks of the survivors again -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["textured", "overlapping"])
def test_a_later_frame_reinserts_what_is_missing(scenes, name):
    s = scenes[name]
    with _fuse(s, 2) as f, _fuse(s, 1, first=2) as fresh:
        st0 = _state(f, s.box); order0 = _stored_inside(f, st0)
        _, _, half = _thresholds(st0, s.box, s)
        params = dict(min_weight=-1.0, box=half)
        counts = f.prune(**params)
        smp = f.debug_frame_samples(s.box, *_args(s.frames[2]))
        assert f.integrate(*_args(s.frames[2])) == 2
        st2 = _state(f, s.box); order2 = _stored_inside(f, st2)
        fr = _state(fresh, s.box); order_fresh = _stored_inside(fresh, fr)
    pruned, gone = _pruned_state(st0, s.box, s.vs, **params)
    want_order = PT.prune(_volume(st0, s.box), order0, voxel_size=s.vs, **params)[1]
    assert counts["removed"] == int(gone.sum()) and 0 < counts["removed"] < counts["stored"]
    # the stored keys: the survivors and what a fresh volume holds after this frame alone
    assert np.array_equal(st2["found"], pruned["found"] | fr["found"])
    back = gone & fr["found"]
    print(f"{name}: {counts['removed']} removed by the box, {int(back.sum())} of them inserted again by the next frame, {int((gone & ~fr['found']).sum())} stay away")
    assert back.sum() > 0
    # the values: the frame's samples on the twin's pruned state, a new voxel starting from Voxel()
    want = DT.integrate(pruned, smp, sel=st2["found"])
    _same_state(st2, _masked(want, st2["found"]), FIELDS)
    # the insertion order: the survivors, then the fresh volume's order less the survivors
    new = order_fresh[~np.isin(LT.pack(order_fresh), LT.pack(want_order))]
    assert np.array_equal(order2, np.concatenate([want_order, new]))
    is_new = st2["found"] & ~pruned["found"]
    assert np.all(st2["first_frame"][is_new] == 2) and np.array_equal(st2["first_frame"][pruned["found"]], st0["first_frame"][pruned["found"]])
    assert np.all(st2["first_frame"][back] == 2)


# ---- 5. frames taken out and moved after a prune ---------------------------------------------------------------------------------------------------------------
def test_deintegrate_and_reintegrate_after_a_prune(scenes):
    s = scenes["overlapping"]
    with _fuse(s, 3) as f:
        st0 = _state(f, s.box)
        wmed, _, _ = _thresholds(st0, s.box, s)
        params = dict(min_weight=wmed)
        counts = f.prune(**params)
        pruned, gone = _pruned_state(st0, s.box, s.vs, **params)
        _same_state(_state(f, s.box), pruned)
        smp0 = f.debug_frame_samples(s.box, *_args(s.frames[0]))
        f.deintegrate(0, *_args(s.frames[0]))
        st1 = _state(f, s.box)
        d, intr, bgr, T, er = s.frames[1]
        T1 = np.array(T, np.float32); T1[:3, 3] += np.array([0.002, -0.0015, 0.001], np.float32)
        smp_old = f.debug_frame_samples(s.box, d, intr, bgr, intr, T, er); smp_new = f.debug_frame_samples(s.box, d, intr, bgr, intr, T1, er)
        assert f.reintegrate(1, d, intr, bgr, intr, T, T1, er) == 3
        st2 = _state(f, s.box); info = f.info()
    assert 0 < counts["removed"] < counts["stored"] and info["frames"] == 4
    # taking frame 0 out skips the voxels that are gone and treats the survivors as before
    want1 = _masked(DT.deintegrate(pruned, smp0, pruned["first_frame"], 0), pruned["found"])
    want1["first_frame"] = pruned["first_frame"]
    _same_state(st1, want1)
    fed = pruned["found"] & smp0["on"] & (pruned["first_frame"] <= 0)
    assert fed.sum() > 500 and (gone & smp0["on"]).sum() > 100 and not st1["found"][gone].any()
    # frame 1 moved: deintegrate + integrate on that state, the cells of the new pose carrying the new ordinal
    assert np.array_equal(st2["found"] & st1["found"], st1["found"]) and np.all(st2["first_frame"][st2["found"] & ~st1["found"]] == 3)
    want2 = _masked(DT.reintegrate(st1, smp_old, smp_new, st2["first_frame"], 1), st2["found"])
    _same_state(st2, want2, FIELDS)
    assert int((st2["found"] & ~st1["found"]).sum()) > 0


# ---- 6. the rebuilt table: shrink, growth across the prune, growth after it, a repeated run ------------------------------------------------------------------------
def test_the_table_shrinks_grows_and_repeats(scenes):
    s = scenes["overlapping"]
    runs = []
    for cap, shrink in ((1, False), (1, True), (1 << 16, False), (1 << 16, True), (1 << 16, True)):
        with _fuse(s, 2, capacity=cap) as f:
            st0 = _state(f, s.box); cap0 = f.info()["capacity"]
            on = st0["found"]
            c = s.box[on].astype(np.float64).mean(0) * s.vs
            column = np.array([c[0] - 4 * s.vs, c[0] + 4 * s.vs, c[1] - 4 * s.vs, c[1] + 4 * s.vs, (s.lo[2] - 1) * s.vs, (s.hi[2] + 1) * s.vs], F)
            counts = f.prune(min_weight=0.0, box=column, shrink=shrink)
            cap1 = f.info()["capacity"]
            st1 = _state(f, s.box); order1 = _stored_inside(f, st1)
            for fr in s.frames[2:]:
                f.integrate(*_args(fr))
            st2 = _state(f, s.box); order2 = _stored_inside(f, st2); cap2 = f.info()["capacity"]
            n = f.finish(0); rec = f.export()
        kept = counts["stored"] - counts["removed"]
        print(f"initial capacity {cap}, shrink {shrink}: capacity {cap0} -> {cap1} -> {cap2}; stored {counts['stored']}, kept {kept}, stored at the end {len(order2)}")
        assert 0 < kept < counts["stored"]
        assert cap1 == PT.capacity_after(cap0, kept, counts["removed"], shrink) <= cap0
        if cap == 1:
            assert cap0 > 4096                                              # the small table grew while fusing
        if shrink:
            assert cap1 == 4096 < cap0 and cap2 > cap1                     # 2 kept <= 4096; the frames that follow make the table grow again
        runs.append((counts, st1, order1, st2, order2, n, rec))
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[5] == runs[0][5]
        _same_state(r[1], runs[0][1]); _same_state(r[3], runs[0][3])
        assert np.array_equal(r[2], runs[0][2]) and np.array_equal(r[4], runs[0][4])
        _same_records(r[6], runs[0][6])


# ---- 7. lane and workgroup edges ---------------------------------------------------------------------------------------------------------------------------------
def _records(s, n, seed=21):
    rng = np.random.default_rng(seed)
    keys = s.box[rng.choice(len(s.box), n, replace=False)]
    return dict(keys=np.ascontiguousarray(keys), sdf=rng.uniform(-0.03, 0.03, n).astype(F), weight=rng.integers(1, 9, n).astype(F),
                color=rng.integers(0, 256, (n, 3)).astype(np.uint8))


def _loaded(s, rec):
    f = B.Fusion(s.vs, 0.1, 10.0, initial_capacity=1 << 12)
    f.insert_records(**rec)
    return f


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_lane_and_workgroup_edges(scenes, n):
    s = scenes["textured"]
    rec = _records(s, n)
    # remove none
    with _loaded(s, rec) as f:
        st0 = _state(f, s.box)
        assert _counts(f.prune(**OFF)) == [n, 0, 0, 0, 0]
        _same_state(_state(f, s.box), st0)
        assert np.array_equal(f.debug_insertion_order(), rec["keys"])
    # remove all: an empty table, and a frame then fuses as into a fresh volume, one ordinal later
    with _loaded(s, rec) as f, B.Fusion(s.vs, 0.1, 10.0, initial_capacity=1 << 12) as fresh:
        assert _counts(f.prune(min_weight=100.0, shrink=bool(n & 1))) == [n, n, n, 0, 0]
        assert not _state(f, s.box)["found"].any() and len(f.debug_insertion_order()) == 0 and f.snapshot() == 0 and len(f.export()["sdf"]) == 0
        assert f.info()["frames"] == 1
        assert f.integrate(*_args(s.frames[0])) == 1 and fresh.integrate(*_args(s.frames[0])) == 0
        a, b = _state(f, s.box), _state(fresh, s.box)
        _same_state(a, b, ("found",) + FIELDS)
        assert a["found"].sum() > 500 and np.all(a["first_frame"][a["found"]] == 1) and np.all(b["first_frame"][b["found"]] == 0)
        assert np.array_equal(f.debug_insertion_order(), fresh.debug_insertion_order())
    # remove exactly one record: the first, the last, and record 64 where there is one
    for i in sorted({0, n - 1} | ({64} if n > 64 else set())):
        one = {k: rec[k].copy() for k in RECORD}; one["weight"][i] = 0.0; one["sdf"][i] = 0.0
        with _loaded(s, one) as f:
            st0 = _state(f, s.box)
            counts = f.prune(shrink=bool(i & 1))
            st1 = _state(f, s.box); order1 = f.debug_insertion_order()
            m = f.snapshot(); snap = f.export()
        want, want_order, want_counts = PT.prune(_volume(st0, s.box), one["keys"], voxel_size=s.vs)
        assert _counts(counts) == want_counts == [n, 1, 1, 0, 0], (n, i)
        got = _volume(st1, s.box)
        for k in ("keys",) + FIELDS + ("first_frame",):
            assert np.array_equal(got[k], want[k]), (n, i, k)
        assert np.array_equal(order1, np.delete(one["keys"], i, 0)) and np.array_equal(order1, want_order), (n, i)
        assert m == n - 1
        _same_records(snap, LT.snapshot_records(_by_key(want), want_order))


# ---- 8. a pruned volume as the source of a general merge ------------------------------------------------------------------------------------------------------------
def test_merge_from_a_pruned_source_equals_the_twin(scenes):
    s = scenes["overlapping"]
    with s.a() as A, s.b() as Bv:
        a0 = FC.snapshot(A, s.box)
        b_st = _state(Bv, s.box); b_order = _stored_inside(Bv, b_st)
        wmed, _, _ = _thresholds(b_st, s.box, s)
        counts = Bv.prune(min_weight=wmed, shrink=True)
        b0 = PT.prune(_volume(b_st, s.box), b_order, voxel_size=s.vs, min_weight=wmed)[0]
        st = A.merge(Bv, FC.POSE)
        R, tv = st["rotation"], st["translation_voxels"]
        lo, hi = FC.moved_box(s.lo, s.hi, R, tv)
        got = FC.snapshot(A, FC.dense(lo, hi))
    assert 0 < counts["removed"] < counts["stored"] and st["aligned"] == 0 and st["ordinal"] == 2
    want, wst = MT.merge(a0, b0, s.vs, 2, R=R, t=FC.POSE[3:], tv=tv)
    assert {k: st[k] for k in ("source_voxels", "sampled", "allocated", "aligned")} == {k: wst[k] for k in ("source_voxels", "sampled", "allocated", "aligned")}, (st, wst)
    assert st["source_voxels"] == len(b0["keys"]) and st["sampled"] > 100
    assert len(got["keys"]) == len(want["keys"]), (len(got["keys"]), len(want["keys"]))
    a, b = np.argsort(DT.pack(got["keys"])), np.argsort(DT.pack(want["keys"]))
    assert np.array_equal(got["keys"][a], want["keys"][b])
    for k in FIELDS + ("first_frame",):
        assert np.array_equal(got[k][a], want[k][b]), (k, int((got[k][a] != want[k][b]).sum()))


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_volume_as_it_was(scenes):
    s = scenes["textured"]
    L = B.load(); p = B._p
    good = np.array([-1.0, 1.0, -1.0, 1.0, -1.0, 1.0], F)
    nan, inf = float("nan"), float("inf")

    def bad_box(i, v):
        b = good.copy(); b[i] = v
        return b
    with _fuse(s, 2) as f:
        st0 = _state(f, s.box); order0 = f.debug_insertion_order(); info0 = f.info()
        sentinel = np.full(5, -7, np.int64)
        assert L.i3d_fusion_prune(None, 0.0, 0.0, 0, None, 0, p(sentinel)) == INVALID
        cases = [((nan, 0.0, 0, None), "finite"), ((inf, 0.0, 0, None), "finite"), ((0.0, nan, 0, None), "finite"), ((0.0, -inf, 0, None), "finite"),
                 ((0.0, 0.0, 3, p(good)), "box_mode"), ((0.0, 0.0, -1, p(good)), "box_mode"), ((0.0, 0.0, 1, None), "null"), ((0.0, 0.0, 2, None), "null")]
        boxes = [bad_box(0, nan), bad_box(5, inf), bad_box(2, -inf), bad_box(0, 2.0), bad_box(3, -2.0), bad_box(4, 1.5)]
        cases += [((0.0, 0.0, 1, p(b)), "finite" if not np.isfinite(b).all() else "lo > hi") for b in boxes]
        for shrink in (0, 1):
            for (mw, ms, mode, box), word in cases:
                assert L.i3d_fusion_prune(f.h, mw, ms, mode, box, shrink, p(sentinel)) == INVALID, (mw, ms, mode, word)
                assert word in L.i3d_fusion_last_error(f.h).decode(), (word, L.i3d_fusion_last_error(f.h).decode())
                assert np.all(sentinel == -7)
        _same_state(_state(f, s.box), st0)
        assert np.array_equal(f.debug_insertion_order(), order0) and f.info() == info0
        # a degenerate box (lo == hi) and null counts are fine
        assert L.i3d_fusion_prune(f.h, -1.0, 0.0, 2, p(np.zeros(6, F) + F(1e3)), 0, None) == OK
        _same_state(_state(f, s.box), st0)
        f.finish(0)
        rec = f.export()
        assert L.i3d_fusion_prune(f.h, 0.0, 0.0, 0, None, 0, p(sentinel)) == ERR_STATE and "finished" in L.i3d_fusion_last_error(f.h).decode()
        assert np.all(sentinel == -7)
        _same_state(_state(f, s.box), st0)
        _same_records(f.export(), rec)
        with pytest.raises(B.I3DError):
            f.prune()


# ---- 10. app_fusion: prune_every / prune_min_weight / prune_max_sdf_voxels -------------------------------------------------------------------------------------------
def test_app_fusion_prune_every(fusion_frames, tmp_path):
    """the three-frame dataset of the other app_fusion tests; the app's file against the file the binding writes for the same sequence of calls"""
    import make_dataset
    app = os.path.join(ROOT, "apps", "app_fusion")
    assert os.path.exists(app), "apps/app_fusion has not been built (run __graft_entry__.build())"
    _, frames, _ = fusion_frames
    sc = dict(voxel_size=FC.VS, intr=FC.INTR, keys=np.zeros((1, 3), np.int32), sdf=np.zeros(1, np.float32), weight=np.ones(1, np.float32), color=np.zeros((1, 3), np.uint8),
              frames=[dict(depth=[d], bgr=[FC.BGR]) for d, _ in frames[:3]], poses=[p for _, p in frames[:3]])
    out = tmp_path / "ds"
    yml, _ = make_dataset.write_dataset(str(out), sc)
    base = (out / "fusion.yml").read_text()
    runs = dict(plain='correct_iterations: "0"\noutput_sdf: "./fusion/plain.tsdf"\n',
                pruned='correct_iterations: "0"\noutput_sdf: "./fusion/pruned.tsdf"\nprune_every: "1"\n',
                band='correct_iterations: "0"\noutput_sdf: "./fusion/band.tsdf"\nprune_every: "2"\nprune_min_weight: "3.5"\nprune_max_sdf_voxels: "3"\n')
    for name, extra in runs.items():
        (out / f"{name}.yml").write_text(base + extra)
        r = subprocess.run([app, "-s", yml, "-f", str(out / f"{name}.yml")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.count("prune after frame") == dict(plain=0, pruned=3, band=1)[name], r.stdout
    (out / "negative.yml").write_text(base + 'prune_every: "-1"\n')
    r = subprocess.run([app, "-s", yml, "-f", str(out / "negative.yml")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "prune_every" in r.stderr
    # the same calls through the binding, on the frames as the app's sensor decodes them
    vs = float(F(float(f"{float(FC.VS):g}")))
    sensor = B.Sensor(out / "rgbd", 0, 0.1, 10.0)                          # sensor.yml's dataset and depth range
    lo, hi = sensor.depth_range
    calls = dict(plain=None, pruned=(1, dict()), band=(2, dict(min_weight=3.5, max_abs_sdf=float(F(3.0) * F(vs)))))
    removed = {}
    for name, how in calls.items():
        with B.Fusion(vs, lo, hi, clip=np.zeros(6, F)) as f:
            removed[name] = 0
            for i in range(3):
                f.integrate(sensor.depth(i), sensor.depth_intrinsics, sensor.color(i), sensor.color_intrinsics, sensor.pose(i), 2)
                if how is not None and (i + 1) % how[0] == 0:
                    removed[name] += f.prune(shrink=True, **how[1])["removed"]
            f.finish(0)
            f.save(tmp_path / f"{name}.tsdf")
        assert (out / "fusion" / f"{name}.tsdf").read_bytes() == (tmp_path / f"{name}.tsdf").read_bytes(), name
    sensor.close()
    print(f"removed through the binding: {removed}")
    assert removed["pruned"] > 0 and removed["band"] > 0
    assert len(B.tsdf_read(out / "fusion" / "band.tsdf")["sdf"]) < len(B.tsdf_read(out / "fusion" / "plain.tsdf")["sdf"])
