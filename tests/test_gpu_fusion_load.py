"""-m gpu: i3d_fusion_insert_records / i3d_fusion_load / i3d_fusion_snapshot on the device, bit for bit: a loaded volume against its records
and the numpy statement (fusion_load_twin.py), every size around a wave and across growth, a resumed run against an uninterrupted one, a snapshot that leaves the
volume as it was, the loaded volume under every reader of the model, the file route with the header's truncation and weight sample, the errors, and app_fusion.

The state of a volume is read with Fusion.debug_voxels over ONE dense box of keys that holds every stored voxel, the weight-0 ones included, so two states over
the box compare element by element."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fusion_cases as FC
import fusion_deintegrate_twin as DT
import fusion_load_twin as LT
from fusion_cases import fusion_frames  # noqa: F401  (fixtures)
from intrinsic3d_amd import binding as B, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

FIELDS = ("sdf", "weight", "color")
RECORD = ("keys", "sdf", "weight", "color")
OK, INVALID, STATE, CAPACITY, IO = 0, 1, 4, 5, 7


def _state(f, box):
    """debug_voxels over the box: found, sdf, weight, color, first_frame, each [len(box)]"""
    return f.debug_voxels(box)


def _same_state(a, b):
    for k in ("found",) + FIELDS + ("first_frame",):
        assert np.array_equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))


def _same_records(a, b):
    assert len(a["sdf"]) == len(b["sdf"]), (len(a["sdf"]), len(b["sdf"]))
    for k in RECORD:
        assert np.array_equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))


def _head(rec, n):
    return {k: rec[k][:n] for k in RECORD}


def _volume(f, box):
    dv = _state(f, box); s = dv["found"]
    return LT.volume_of(box[s], dv["sdf"][s], dv["weight"][s], dv["color"][s], dv["first_frame"][s])


class Scene:
    """the three textured frames of the merge tests, the box, and what several tests start from, each computed once and never written to"""

    def __init__(self):
        sc, fr = FC.textured_frames(seed=5, K=3, radius=10, w=96, h=72)
        self.sc, self.vs = sc, float(sc["voxel_size"])
        self.intr = sc["intr"].astype(np.float32)
        self.frames = [(d, self.intr, bgr, self.intr, T, 2) for d, bgr, T in fr]
        self.poses = [np.asarray(p, np.float64) for p in sc["poses"]]
        self.h, self.w = fr[0][0].shape
        with self.fused(3) as f:
            self.order_u = f.debug_insertion_order()                       # every stored voxel of the uninterrupted run, in insertion order
            self.n0 = f.snapshot(); self.r0 = f.export()                   # = finish(0)
            f.finish(10); self.r10 = f.export()
        self.lo = self.order_u.min(0).astype(np.int64) - 2; self.hi = self.order_u.max(0).astype(np.int64) + 3
        self.box = FC.dense(self.lo, self.hi)
        with self.fused(3) as f:
            self.state_u = _state(f, self.box)
        assert int(self.state_u["found"].sum()) == len(self.order_u) > len(self.r0["sdf"]) > 3000

    def empty(self, capacity=1 << 16):
        return B.Fusion(self.vs, 0.1, 10.0, initial_capacity=capacity)

    def fused(self, n, capacity=1 << 16, first=0):
        f = self.empty(capacity)
        for fr in self.frames[first:first + n]:
            f.integrate(*fr)
        return f

    def loaded(self, rec, capacity=1 << 16):
        f = self.empty(capacity)
        f.insert_records(**{k: rec[k] for k in RECORD})
        return f

    def camera(self, i=1):
        return dict(width=self.w, height=self.h, intr=self.sc["intr"], pose=self.poses[i])


@pytest.fixture(scope="module")
def S():
    return Scene()


def _key_set(keys):
    return set(LT.pack(keys).tolist())


def _check_loaded(S, L, rec):
    """the volume L holds exactly the records, as given, all first inserted by ordinal 0, in the order given"""
    st = _state(L, S.box)
    assert np.array_equal(st["found"], np.isin(LT.pack(S.box), LT.pack(rec["keys"])))
    assert int(st["found"].sum()) == len(rec["sdf"])
    got = DT.lookup(rec, S.box[st["found"]])
    assert got["found"].all()
    for k in FIELDS:
        assert np.array_equal(st[k][st["found"]], got[k]), k
    assert np.all(st["first_frame"][st["found"]] == 0) and np.all(st["first_frame"][~st["found"]] == -1)
    assert L.info()["frames"] == 1
    assert np.array_equal(L.debug_insertion_order(), np.asarray(rec["keys"], np.int32).reshape(-1, 3))
    return st


# ---- 1. load only ---------------------------------------------------------------------------------------------------------------------------------------------
def test_load_only(S):
    R = S.r10
    assert len(R["sdf"]) > 3000 and np.all(R["weight"] > 0)
    with S.loaded(R) as L:
        _check_loaded(S, L, R)
        n = L.snapshot()
        snap = L.export()
        want = LT.snapshot_records(LT.loaded(R), R["keys"])
        assert n == len(R["sdf"])
        _same_records(snap, want)
        assert not np.array_equal(snap["keys"], R["keys"])                 # the reference reorders on load (limit 2), and so does this
        assert L.finish(0) == n
        _same_records(L.export(), snap)


def test_weightless_records_are_stored_and_not_saved(S):
    R = {k: S.r10[k][:500].copy() for k in RECORD}
    R["weight"][::7] = 0.0; R["sdf"][::7] = 0.0
    with S.loaded(R) as L:
        _check_loaded(S, L, R)                                              # allocated, empty
        assert L.snapshot() == int((R["weight"] > 0).sum())
        _same_records(L.export(), LT.snapshot_records(LT.loaded(R), R["keys"]))


# ---- 2. sizes around a wave, and across several growths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, -1])
def test_sizes_and_growth(S, n):
    R = _head(S.r10, len(S.r10["sdf"]) if n < 0 else n)
    with S.loaded(R, capacity=1) as small, S.loaded(R) as big:
        a = _check_loaded(S, small, R); b = _check_loaded(S, big, R)
        _same_state(a, b)
        assert small.info()["capacity"] >= len(R["sdf"]) / 0.6 and (n >= 0 or small.info()["capacity"] > 4096)      # the small table grew before the launch
        na, nb = small.snapshot(), big.snapshot()
        assert na == nb == len(R["sdf"])
        snap = small.export()
        _same_records(snap, big.export())
        _same_records(snap, LT.snapshot_records(LT.loaded(R), R["keys"]))


# ---- 3. resume: frames 0, 1 | checkpoint | load | frame 2 against frames 0, 1, 2 --------------------------------------------------------------------------------
def test_resume_equals_uninterrupted(S):
    with S.fused(2) as C0:
        C0.snapshot(); ck = C0.export()
    with S.loaded(ck) as Cv, S.fused(1, first=2) as G:
        assert Cv.integrate(*S.frames[2]) == 1                            # the load was ordinal 0
        c = _state(Cv, S.box); order_c = Cv.debug_insertion_order(); order_g = G.debug_insertion_order()
        vol_c = _volume(Cv, S.box)
        Cv.snapshot(); snap_c = Cv.export()
    u = S.state_u
    on_u, on_c = u["found"] & (u["weight"] > 0), c["found"] & (c["weight"] > 0)
    print(f"weight > 0: uninterrupted {int(on_u.sum())}, resumed {int(on_c.sum())}, only uninterrupted {int((on_u & ~on_c).sum())}, only resumed {int((~on_u & on_c).sum())}")
    assert np.array_equal(on_u, on_c)
    for k in FIELDS:
        assert np.array_equal(u[k][on_u], c[k][on_c]), (k, int((u[k][on_u] != c[k][on_c]).sum()))
    assert int(c["found"].sum()) == len(order_c)
    # the snapshot against the twin, on the device's own insertion sequence
    _same_records(snap_c, LT.snapshot_records(vol_c, order_c))
    # the insertion sequence itself: the file's order, then what frame 2 alone inserts, less what the checkpoint already held
    have = _key_set(ck["keys"])
    new = order_g[~np.isin(LT.pack(order_g), LT.pack(ck["keys"]))]
    assert len(new) > 50 and len(have) == len(ck["sdf"])
    assert np.array_equal(order_c, np.concatenate([ck["keys"], new]))
    assert np.all(c["first_frame"][np.isin(LT.pack(S.box), LT.pack(new))] == 1)
    # the same statement on the uninterrupted volume: the new debug entry against the existing path
    s = u["found"]
    vol_u = LT.volume_of(S.box[s], u["sdf"][s], u["weight"][s], u["color"][s], u["first_frame"][s])
    _same_records(S.r0, LT.snapshot_records(vol_u, S.order_u))


# ---- 4. a snapshot leaves the volume open and untouched -----------------------------------------------------------------------------------------------------------
def test_snapshot_leaves_the_volume_open_and_untouched(S, tmp_path):
    L = B.load()
    near = S.r0["keys"][::3][:2000]
    pts = (near + np.random.default_rng(4).uniform(-0.4, 0.4, near.shape)) * S.vs
    with S.fused(2) as A, S.fused(2) as Plain:
        sentinel = np.full(8, -7.0, np.float32)
        assert L.i3d_fusion_get(A.h, None, B._p(sentinel), None, None) == STATE and np.all(sentinel == -7.0)
        assert L.i3d_fusion_save(A.h, str(tmp_path / "no.tsdf").encode()) == STATE and not (tmp_path / "no.tsdf").exists()
        before = (_state(A, S.box), A.render(S.camera()), A.query_points(pts), A.info())
        n = A.snapshot()
        snap = A.export()
        after = (_state(A, S.box), A.render(S.camera()), A.query_points(pts), A.info())
        _same_state(before[0], after[0])
        for k in ("depth", "normal"):
            assert np.array_equal(before[1][k], after[1][k]), k
        assert before[1]["stats"]["hits"] == after[1]["stats"]["hits"] > 300
        for k in ("sdf", "normal", "status"):
            assert np.array_equal(before[2][k], after[2][k], equal_nan=True), k
        assert {k: v for k, v in before[3].items() if k != "allocated"} == {k: v for k, v in after[3].items() if k != "allocated"}
        assert after[3]["frames"] == 2 and n == len(snap["sdf"]) > 3000
        with S.fused(2) as F0:
            assert F0.finish(0) == n
            _same_records(F0.export(), snap)                              # the records finish(0) would produce
        assert A.integrate(*S.frames[2]) == 2 and Plain.integrate(*S.frames[2]) == 2
        _same_records(A.export(), snap)                                    # still the snapshot
        A.save(tmp_path / "snap.tsdf")
        _same_records(B.tsdf_read(tmp_path / "snap.tsdf"), snap)
        _same_state(_state(A, S.box), _state(Plain, S.box))
        _same_state(_state(A, S.box), S.state_u)
        assert A.finish(10) == Plain.finish(10) == len(S.r10["sdf"])
        _same_records(A.export(), S.r10)
        _same_records(Plain.export(), S.r10)
        assert A.snapshot() == len(S.r10["sdf"])                           # on a finished volume: the finished count
        _same_records(A.export(), S.r10)


# ---- 5. the loaded volume as a model ----------------------------------------------------------------------------------------------------------------------------------
def _camera_rays(S, i):
    """the pixel rays of camera i in world coordinates (pose = world -> camera, angle-axis | t)"""
    p = S.poses[i]; R = synthetic.aa_to_rotmat(p[:3]); fx, fy, cx, cy = [float(x) for x in S.sc["intr"]]
    v, u = np.mgrid[0:S.h, 0:S.w]
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, np.float64)], -1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(-R.T @ p[3:], (len(d), 1)), d @ R


def test_loaded_volume_is_the_live_one_to_every_reader(S):
    rng = np.random.default_rng(11)
    sel = rng.choice(len(S.r0["sdf"]), 2000, replace=False)
    pts = (S.r0["keys"][sel] + rng.uniform(-0.5, 0.5, (2000, 3))) * S.vs
    o, d = _camera_rays(S, 1)
    start = S.poses[2] + np.array([0.004, -0.003, 0.002, 0.003, -0.002, 0.004])
    with S.loaded(S.r0) as Lv, S.fused(3) as O:
        a, b = Lv.render(S.camera()), O.render(S.camera())
        assert a["stats"]["hits"] == b["stats"]["hits"] > 300
        for k in ("depth", "normal"):
            assert np.array_equal(a[k], b[k]), k
        a, b = Lv.cast_rays(o, d), O.cast_rays(o, d)
        assert int((a["status"] == b["status"]).all()) and a["stats"]["hits"] == b["stats"]["hits"] > 300
        for k in ("t", "position", "normal", "status"):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        a, b = Lv.query_points(pts), O.query_points(pts)
        assert a["stats"] == b["stats"]
        for k in ("sdf", "normal", "status"):
            assert np.array_equal(a[k], b[k], equal_nan=True), k
        assert np.isfinite(a["sdf"]).sum() > 500
        a, b = Lv.extract_mesh(), O.extract_mesh()
        assert len(a[0]) > 500 and len(a[2]) > 500
        for x, y, name in zip(a, b, ("vertices", "colors", "faces")):
            assert np.array_equal(x, y), name
        (pa, sa), (pb, sb) = Lv.track_sdf(S.frames[2][0], start, S.sc["intr"]), O.track_sdf(S.frames[2][0], start, S.sc["intr"])
        assert np.array_equal(pa, pb) and sa == sb and sa["valid"] > 300
        # as the source of a merge into copies of a one-frame volume
        lo, hi = FC.moved_box(S.lo, S.hi, synthetic.aa_to_rotmat(FC.POSE[:3]), FC.POSE[3:] / S.vs)
        box = FC.dense(lo, hi)
        with S.fused(1) as D1, S.fused(1) as D2:
            s1, s2 = D1.merge(Lv, FC.POSE), D2.merge(O, FC.POSE)
            assert {k: s1[k] for k in FC.COUNTS} == {k: s2[k] for k in FC.COUNTS} and s1["allocated"] > 100 and s1["aligned"] == 0
            _same_state(_state(D1, box), _state(D2, box))


# ---- 6. the file route ------------------------------------------------------------------------------------------------------------------------------------------------
def test_file_route_equals_the_records_route(S, tmp_path):
    p = tmp_path / "volume.tsdf"
    with S.fused(3) as O:
        O.snapshot(); O.save(p); rec = O.export()
    with B.Fusion.load(p, 0.1, 10.0) as F, S.loaded(rec) as Lv:
        _same_state(_state(F, S.box), _state(Lv, S.box))
        assert F.info()["frames"] == 1 and F.snapshot() == Lv.snapshot()
        _same_records(F.export(), Lv.export())
        assert np.array_equal(F.debug_insertion_order(), rec["keys"])


def test_truncation_and_weight_sample_come_from_the_header(S, tmp_path):
    """A header with truncation 4 vs and weight sample 7 (a fresh volume has 5 vs and 10): both are written back by save, and both drive the next integrate - the
    gate sdf > -truncation and the weights, each at most the weight sample (their mean of three, floored at 3).  A weight sample of 0 gives unit weights."""
    vs = np.float32(S.vs); tr = float(np.float32(4.0) * vs)
    with S.fused(2) as C0:
        C0.snapshot(); ck = C0.export()
    p, q, z = tmp_path / "in.tsdf", tmp_path / "out.tsdf", tmp_path / "zero.tsdf"
    B.tsdf_write(p, S.vs, ck["keys"], ck["sdf"], ck["weight"], ck["color"], truncation=tr, integration_weight_sample=7.0)
    B.tsdf_write(z, S.vs, ck["keys"], ck["sdf"], ck["weight"], ck["color"])
    with B.Fusion.load(p, 0.1, 10.0) as F, S.loaded(ck) as D, B.Fusion.load(z, 0.1, 10.0) as Z:
        F.snapshot(); F.save(q)
        hdr = B.tsdf_read(q)
        assert hdr["truncation"] == np.float32(tr) and hdr["integration_weight_sample"] == np.float32(7.0) and hdr["voxel_size"] == vs
        _same_records(hdr, LT.snapshot_records(LT.loaded(ck), ck["keys"]))
        smp = F.debug_frame_samples(S.box, *S.frames[2]); dflt = D.debug_frame_samples(S.box, *S.frames[2]); unit = Z.debug_frame_samples(S.box, *S.frames[2])
        assert smp["on"].sum() > 500 and np.all(smp["sample"][smp["on"]] > -np.float32(tr)) and np.all(smp["wu"][smp["on"]] <= 7.0) and np.all(smp["wu"][smp["on"]] >= 3.0)
        cut = dflt["on"] & ~smp["on"]
        assert cut.sum() > 20 and np.all(dflt["sample"][cut] <= -np.float32(tr)) and dflt["wu"][dflt["on"]].max() > 7.0
        assert np.array_equal(unit["on"], dflt["on"]) and np.all(unit["wu"][unit["on"]] == 1.0)
        for f, s in ((F, smp), (Z, unit)):
            before = _state(f, S.box)
            assert f.integrate(*S.frames[2]) == 1
            after = _state(f, S.box)
            want = DT.integrate(before, s, sel=after["found"])                # a voxel the frame inserted starts from Voxel(): zeros, as the lookup gives
            for k in FIELDS:
                assert np.array_equal(after[k], want[k]), k
            assert int((s["on"] & after["found"]).sum()) > 500


# ---- 7. errors ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_errors(S, tmp_path):
    L = B.load(); p = B._p
    R = {k: np.ascontiguousarray(S.r10[k][:300]) for k in RECORD}
    n = 300

    def raw(f, rec=R, n=n, **null):
        a = [None if k in null else p(np.ascontiguousarray(rec[k])) for k in RECORD]
        return L.i3d_fusion_insert_records(f.h if f is not None else None, n, *a)

    def is_empty(f):
        assert f.info()["frames"] == 0 and len(f.debug_insertion_order()) == 0 and not _state(f, S.box)["found"].any()

    def changed(k, i, value):
        rec = {q: R[q].copy() for q in RECORD}; rec[k][i] = value
        return rec
    with S.empty() as f:
        assert raw(None) == INVALID
        for k in RECORD:
            assert raw(f, **{k: True}) == INVALID and "null" in L.i3d_fusion_last_error(f.h).decode(); is_empty(f)
        assert raw(f, n=(1 << 30) + 1) == INVALID and "2^30" in L.i3d_fusion_last_error(f.h).decode(); is_empty(f)
        for k, i, value, word in (("keys", (5, 1), 1 << 20, "2^20"), ("keys", (299, 2), -(1 << 20), "2^20"), ("sdf", 7, np.nan, "sdf"), ("sdf", 0, np.inf, "sdf"),
                                  ("weight", 9, np.nan, "weight"), ("weight", 299, np.inf, "weight"), ("weight", 64, -1.0, "weight")):
            assert raw(f, changed(k, i, value)) == INVALID and word in L.i3d_fusion_last_error(f.h).decode(), (k, i, value); is_empty(f)
        assert raw(f, n=0, keys=True, sdf=True, weight=True, color=True) == OK and f.info()["frames"] == 1 and len(f.debug_insertion_order()) == 0
        assert raw(f) == STATE                                              # an empty load is a load
    # a key twice: refused on the device, the volume empty again, and a correct load then is the load of test 1
    for i, j in ((0, n - 1), (64, 65)):
        with S.empty(capacity=1) as f:
            assert raw(f, changed("keys", j, R["keys"][i])) == INVALID and "twice" in L.i3d_fusion_last_error(f.h).decode(), (i, j)
            is_empty(f)
            assert raw(f) == OK
            _check_loaded(S, f, R)
    with S.loaded(R) as f:
        before = _state(f, S.box); info = f.info()
        assert raw(f) == STATE and "not empty" in L.i3d_fusion_last_error(f.h).decode()                    # a second load
        d, intr, bgr, cintr, T, er = S.frames[0]
        assert L.i3d_fusion_deintegrate(f.h, 0, S.w, S.h, p(intr), S.w, S.h, p(intr), p(d), p(bgr), p(T), er) == STATE      # the load's ordinal is never live
        _same_state(before, _state(f, S.box)); assert f.info() == info
        order = f.debug_insertion_order(); cnt = C.c_uint64(0); out = np.full((n, 3), -9, np.int32)
        assert L.i3d_fusion_debug_insertion_order(f.h, n - 1, p(out), C.byref(cnt)) == CAPACITY and cnt.value == n and np.all(out == -9)
        assert L.i3d_fusion_debug_insertion_order(f.h, n, p(out), C.byref(cnt)) == OK and np.array_equal(out, order)
        f.finish(0)
    with S.fused(1) as f:
        before = _state(f, S.box)
        assert raw(f) == STATE and "not empty" in L.i3d_fusion_last_error(f.h).decode()                    # a load after integrate
        _same_state(before, _state(f, S.box)); assert f.info()["frames"] == 1
    with S.empty() as f:
        assert f.finish(0) == 0
        assert raw(f) == STATE and "finished" in L.i3d_fusion_last_error(f.h).decode()                     # a load after finish
    # the file route
    good = tmp_path / "good.tsdf"
    B.tsdf_write(good, S.vs, R["keys"], R["sdf"], R["weight"], R["color"])
    cut = tmp_path / "cut.tsdf"; cut.write_bytes(good.read_bytes()[:24 + 24 * 10 + 11])                   # in the middle of record 10
    zero = tmp_path / "zero.tsdf"
    B.tsdf_write(zero, 0.0, R["keys"], R["sdf"], R["weight"], R["color"])
    twice = tmp_path / "twice.tsdf"
    B.tsdf_write(twice, S.vs, changed("keys", 65, R["keys"][64])["keys"], R["sdf"], R["weight"], R["color"])
    for path, code in ((tmp_path / "missing.tsdf", IO), (cut, IO), (zero, IO), (twice, INVALID)):
        h = C.c_void_p(12345)
        assert L.i3d_fusion_load(0, str(path).encode(), 0.1, 10.0, None, C.byref(h)) == code and not h.value, path
        with pytest.raises(B.I3DError):
            B.Fusion.load(path, 0.1, 10.0)
    h = C.c_void_p(12345)
    assert L.i3d_fusion_load(99, str(good).encode(), 0.1, 10.0, None, C.byref(h)) == 2 and not h.value     # I3D_ERR_NO_DEVICE as i3d_fusion_create
    with B.Fusion.load(good, 0.1, 10.0) as f:
        _check_loaded(S, f, R)


# ---- 8. app_fusion: checkpoint_every / checkpoint_volume / resume_volume ------------------------------------------------------------------------------------------------
def test_app_fusion_checkpoint_and_resume(fusion_frames, tmp_path):
    """the dataset of test_app_fusion_repose_passes, its first three frames (the textured scene lies nearer than the sensor's min_depth)"""
    import make_dataset
    app = os.path.join(ROOT, "apps", "app_fusion")
    assert os.path.exists(app), "apps/app_fusion has not been built (run __graft_entry__.build())"
    _, frames, _ = fusion_frames
    sc = dict(voxel_size=FC.VS, intr=FC.INTR, keys=np.zeros((1, 3), np.int32), sdf=np.zeros(1, np.float32), weight=np.ones(1, np.float32), color=np.zeros((1, 3), np.uint8),
              frames=[dict(depth=[d], bgr=[FC.BGR]) for d, _ in frames[:3]], poses=[p for _, p in frames[:3]])
    out = tmp_path / "ds"
    yml, _ = make_dataset.write_dataset(str(out), sc)
    base = (out / "fusion.yml").read_text()
    B.keyframes_save(str(out / "fusion" / "after.txt"), 1, np.ones(3), np.array([0, 0, 1], np.uint8))
    runs = dict(plain='correct_iterations: "0"\noutput_sdf: "./fusion/plain.tsdf"\n',
                full='correct_iterations: "0"\noutput_sdf: "./fusion/full.tsdf"\ncheckpoint_every: "2"\ncheckpoint_volume: "./fusion/checkpoint.tsdf"\n',
                resumed='correct_iterations: "0"\noutput_sdf: "./fusion/resumed.tsdf"\nresume_volume: "./fusion/checkpoint.tsdf"\nkeyframes: "./fusion/after.txt"\n')
    for name, extra in runs.items():
        (out / f"{name}.yml").write_text(base + extra)
        r = subprocess.run([app, "-s", yml, "-f", str(out / f"{name}.yml")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("checkpoint after frame 1" in r.stdout) == (name == "full") and ("Resuming" in r.stdout) == (name == "resumed"), r.stdout
        assert r.stdout.count("integrating frame") == (1 if name == "resumed" else 3), r.stdout
    assert (out / "fusion" / "plain.tsdf").read_bytes() == (out / "fusion" / "full.tsdf").read_bytes()      # checkpoints leave the run as it was
    full, res, ck = (B.tsdf_read(out / "fusion" / f"{n}.tsdf") for n in ("full", "resumed", "checkpoint"))
    assert len(ck["sdf"]) > 500 and len(full["sdf"]) > len(ck["sdf"])
    a, b = np.argsort(LT.pack(full["keys"])), np.argsort(LT.pack(res["keys"]))
    print(f"records: full run {len(a)}, resumed run {len(b)}")
    assert len(a) == len(b)
    for k in RECORD:
        assert np.array_equal(full[k][a], res[k][b]), k
    # a voxel size that is not the file's, bit for bit, is refused
    (out / "other.yml").write_text(base + 'voxel_size: "0.0123"\nresume_volume: "./fusion/checkpoint.tsdf"\n')
    r = subprocess.run([app, "-s", yml, "-f", str(out / "other.yml")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "voxel size" in r.stderr
