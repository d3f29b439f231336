"""-m gpu: i3d_fusion_merge on the device against its numpy statement (fusion_merge_twin.py), bit for bit over every stored voxel: the aligned
path under the identity and under lattice translations, the general path under an oblique rotation into an empty and into a populated volume, growth and
reproducibility of the ranks, the interplay with deintegrate / integrate (section 23), that nothing else moves, and the errors.

The state of a volume is read with Fusion.debug_voxels over a dense box of keys that holds all its stored voxels, those of weight 0 included (the box is checked
against the number of voxels a finished copy reports)."""
import ctypes as C

import numpy as np
import pytest

import fusion_deintegrate_twin as DT
import fusion_merge_twin as MT
import query_twin as QT
from fusion_cases import COUNTS, FIELDS, INTR, POSE, VS, VS2, dense, fuse, moved_box, same_render, snapshot
from fusion_cases import fusion_frames, scenes  # noqa: F401  (fixtures)
from intrinsic3d_amd import binding as B, synthetic

pytestmark = pytest.mark.gpu


def _same_volume(got, want):
    assert len(got["keys"]) == len(want["keys"]), (len(got["keys"]), len(want["keys"]))
    a, b = np.argsort(DT.pack(got["keys"])), np.argsort(DT.pack(want["keys"]))
    assert np.array_equal(got["keys"][a], want["keys"][b])
    for k in FIELDS:
        assert np.array_equal(got[k][a], want[k][b]), (k, int((got[k][a] != want[k][b]).sum()))


def _first_frame_at(vol, keys):
    """the first frame of the volume's voxels at keys [n, 3]; -1 where the key is not stored"""
    have = DT.pack(vol["keys"]); order = np.argsort(have); want = DT.pack(keys)
    pos = np.minimum(np.searchsorted(have[order], want), max(0, have.size - 1))
    return np.where(have[order][pos] == want, vol["first_frame"][order][pos], -1) if have.size else np.full(len(want), -1, np.int64)


def _check_counts(st, want):
    assert {k: st[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, (st, want)


# ---- 1. aligned, identity -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["overlapping", "textured"])
def test_aligned_identity_equals_twin(scenes, name):
    s = scenes[name]
    with s.a() as A, s.b() as Bv:
        a0, b0 = snapshot(A, s.box), snapshot(Bv, s.box)
        st = A.merge(Bv)
        got = snapshot(A, s.box)
        assert A.info()["frames"] == 3
    want, wst = MT.merge(a0, b0, s.vs, 2, m=(0, 0, 0))
    _same_volume(got, want)
    _check_counts(st, wst)
    assert st["aligned"] == 1 and st["ordinal"] == 2 and np.array_equal(st["rotation"], np.eye(3)) and not st["translation_voxels"].any()
    missing = ~DT.lookup(a0, b0["keys"])["found"] & (b0["weight"] != 0)
    assert st["allocated"] == int(missing.sum()) > 20 and st["sampled"] == int((b0["weight"] != 0).sum()) > st["allocated"]
    assert np.all(_first_frame_at(got, b0["keys"][missing]) == 2) and int((got["first_frame"] == 2).sum()) == st["allocated"]      # M exactly on the inserted keys
    print(f"{name}: {st['source_voxels']} source voxels, {st['sampled']} sampled, {st['allocated']} inserted")


# ---- 2. aligned, a lattice translation into an empty volume ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [(5, -3, 2), (-70, -65, -80)])
def test_lattice_translation_into_empty(scenes, m):
    s = scenes["pow2"]; m = np.array(m, np.int64)
    with B.Fusion(VS2, 0.1, 10.0, initial_capacity=1 << 16) as A, s.b() as Bv:
        b0 = snapshot(Bv, s.box)
        st = A.merge(Bv, np.concatenate([np.zeros(3), m * VS2]))
        got = snapshot(A, dense(s.lo + m, s.hi + m))
        assert A.info()["frames"] == 1
    on = b0["weight"] != 0
    assert st["aligned"] == 1 and np.array_equal(st["translation_voxels"], m.astype(np.float64)) and st["allocated"] == st["sampled"] == int(on.sum()) > 1000
    order = np.argsort(DT.pack(got["keys"])); want = np.argsort(DT.pack(b0["keys"][on] + m))
    assert np.array_equal(got["keys"][order], (b0["keys"][on] + m)[want])
    assert np.array_equal(got["weight"][order], b0["weight"][on][want])
    assert np.array_equal(got["sdf"][order], ((b0["sdf"][on] * b0["weight"][on]) / b0["weight"][on])[want])
    assert np.all(got["first_frame"] == 0) and (m[0] > 0 or (got["keys"] < 0).all(1).any())
    _same_volume(got, MT.merge(MT.volume(), b0, VS2, 0, m=m)[0])


# ---- 3. general -------------------------------------------------------------------------------------------------------------------------------------------------
def _surface_points(fusion_frames):
    scene, _, pts = fusion_frames
    p = pts[np.isfinite(pts).all(1)].copy()
    for _ in range(4):                                                           # onto the ground-truth surface along the radius
        d = p - scene.c
        p = p - scene.sdf(p)[:, None] * d / np.sqrt((d * d).sum(1, keepdims=True))
    return p


@pytest.mark.parametrize("into", ["empty", "populated"])
def test_general_equals_twin(scenes, fusion_frames, into):
    s = scenes["overlapping"]
    pts = _surface_points(fusion_frames)
    with (s.a() if into == "populated" else B.Fusion(VS, 0.1, 10.0, initial_capacity=1 << 16)) as A, s.b() as Bv:
        a0, b0 = snapshot(A, s.box), snapshot(Bv, s.box)
        M = A.info()["frames"]
        st = A.merge(Bv, POSE)
        R, tv = st["rotation"], st["translation_voxels"]
        lo, hi = moved_box(s.lo, s.hi, R, tv)
        got = snapshot(A, dense(lo, hi))
        moved = pts @ R.T + POSE[3:]
        dev = A.query_points(moved, project=0)["stats"]
        own = Bv.query_points(pts, project=0)["stats"]
    assert st["aligned"] == 0 and st["ordinal"] == M == (2 if into == "populated" else 0)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-14 and np.array_equal(tv, POSE[3:] / VS)
    want, wst = MT.merge(a0, b0, VS, M, R=R, t=POSE[3:], tv=tv)
    _same_volume(got, want)
    _check_counts(st, wst)
    assert st["allocated"] > 1000 and st["sampled"] >= st["allocated"]
    tw = QT.query(QT.Grid(want["keys"], want["sdf"].astype(np.float64), want["weight"], VS), moved, project=False)["stats"]
    print(f"general merge into {into}: {st['source_voxels']} source voxels, {st['sampled']} sampled, {st['allocated']} inserted; moved surface points: "
          f"{dev['valid']} valid, mean |sdf| {dev['sum_abs_sdf'] / max(1, dev['valid']):.6e} m (twin {tw['sum_abs_sdf'] / max(1, tw['valid']):.6e}); "
          f"the source's own: {own['valid']} valid, mean |sdf| {own['sum_abs_sdf'] / max(1, own['valid']):.6e} m")
    assert dev["valid"] == tw["valid"] > 500
    assert abs(dev["sum_abs_sdf"] - tw["sum_abs_sdf"]) <= 1e-9 * tw["sum_abs_sdf"]


# ---- 4. growth and reproducibility --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["aligned", "general"])
def test_growth_and_reproducibility(scenes, path):
    s = scenes["overlapping"]
    pose = None if path == "aligned" else POSE
    runs = []
    for cap in (1 << 10, 1 << 16, 1 << 16):
        # aligned: frame 2's volume into frames 0-1, whose 4096-slot table has grown twice before the merge; general: the volume of all four frames into an
        # empty 4096-slot table, so that the table grows inside the merge and the allocation launch is repeated
        with (s.a(cap) if path == "aligned" else B.Fusion(VS, 0.1, 10.0, initial_capacity=cap)) as A, (s.b() if path == "aligned" else fuse(s.frames, VS)) as Bv:
            before = A.info()["capacity"]
            st = A.merge(Bv, pose)
            lo, hi = moved_box(s.lo, s.hi, st["rotation"], st["translation_voxels"])
            dv = A.debug_voxels(dense(lo, hi))
            grown = A.info()["capacity"] // before
            ex = A.export()
        runs.append((dv, ex, st, grown, before))
    if path == "general":
        assert runs[0][4] == 4096 and runs[0][2]["allocated"] > 0.6 * 4096 and runs[0][3] >= 2 and runs[1][3] == 1, [r[3:] for r in runs]
    else:
        assert 4096 < runs[0][4] < runs[1][4] and runs[1][3] == 1, [r[3:] for r in runs]
    for dv, ex, st, _, _ in runs[1:]:
        for k in ("found",) + FIELDS:
            assert np.array_equal(dv[k], runs[0][0][k]), k
        for k in ("keys", "sdf", "weight", "color"):
            assert np.array_equal(ex[k], runs[0][1][k]), k
        assert {k: st[k] for k in COUNTS} == {k: runs[0][2][k] for k in COUNTS}
    assert runs[0][0]["found"].sum() > 1000 and len(runs[0][1]["sdf"]) > 1000


# ---- 5. with section 23 --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["aligned", "general"])
def test_deintegrate_and_integrate_after_a_merge(scenes, fusion_frames, path):
    s = scenes["overlapping"]
    # general: the same rotation about the sphere's centre and a few voxels off it, so that the merged-in voxels stay where the frames look (the twin on the
    # oracle's volumes inserts 472 voxels under this pose; about the centre alone only 9, the blocks of frames 0-1 cover the rest)
    c = fusion_frames[0].c; Rc = synthetic.aa_to_rotmat(POSE[:3])
    pose = None if path == "aligned" else np.concatenate([POSE[:3], c - Rc @ c + np.array([2.3, -1.7, 3.1]) * VS])
    args = lambda i: (s.frames[i][0], s.frames[i][1], s.frames[i][2], s.frames[i][1], s.frames[i][3], s.frames[i][4])  # noqa: E731
    with s.a() as A, s.a() as A2, s.b() as Bv:
        st = A.merge(Bv, pose); A2.merge(Bv, pose)
        lo, hi = moved_box(s.lo, s.hi, st["rotation"], st["translation_voxels"])
        box = dense(lo, hi)
        merged = snapshot(A, box)
        _same_volume(merged, snapshot(A2, box))
        keys = np.ascontiguousarray(merged["keys"], np.int32)
        inserted = merged["first_frame"] == 2
        assert st["ordinal"] == 2 and int(inserted.sum()) == st["allocated"] > 20
        # an earlier frame leaves: the twin's removal on the merged state; the merged-in voxels are skipped although the frame's gates pass on some of them
        smp = A.debug_frame_samples(keys, *args(0))
        A.deintegrate(0, *args(0))
        got = A.debug_voxels(keys)
        want = DT.deintegrate(merged, smp, merged["first_frame"], 0)
        for k in ("sdf", "weight", "color"):
            assert np.array_equal(got[k], want[k]), k
            assert np.array_equal(got[k][inserted], merged[k][inserted]), k
        assert got["found"].all() and np.array_equal(got["first_frame"], merged["first_frame"])
        fed = smp["on"] & ~inserted
        print(f"{path}: frame 0 out after the merge: {int(fed.sum())} voxels fed, {int((smp['on'] & inserted).sum())} merged-in voxels passed its gates and were skipped")
        assert fed.sum() > 1000
        # a later frame comes in: integrate's update on the merged state, the merged-in voxels included
        assert A2.integrate(*args(3)) == 3
        after = snapshot(A2, box)
        k2 = np.ascontiguousarray(after["keys"], np.int32)
        smp = A2.debug_frame_samples(k2, *args(3))
        base = DT.lookup(merged, k2)
        want = DT.integrate(base, smp)
        for k in ("sdf", "weight", "color"):
            assert np.array_equal(after[k], want[k]), k
        was = _first_frame_at(merged, k2)
        assert np.array_equal(after["first_frame"], np.where(was >= 0, was, 3))
        assert int((smp["on"] & (was == 2)).sum()) >= 10                                             # it feeds voxels the merge inserted
        # the merge's own ordinal is never live
        L = B.load(); p = B._p; d, intr, bgr, _, T, er = args(2); h, w = d.shape
        for f in (A, A2):
            before = f.debug_voxels(keys)
            assert L.i3d_fusion_deintegrate(f.h, 2, w, h, p(intr), w, h, p(intr), p(d), p(bgr), p(T), er) == 4
            assert "ordinal 2" in L.i3d_fusion_last_error(f.h).decode()
            now = f.debug_voxels(keys)
            assert all(np.array_equal(before[k], now[k]) for k in FIELDS)


# ---- 6. nothing else moves -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["aligned", "general"])
def test_nothing_else_moves(scenes, fusion_frames, path):
    s = scenes["overlapping"]
    _, frames, _ = fusion_frames
    pose = None if path == "aligned" else POSE
    h, w = s.frames[0][0].shape
    cam = dict(width=w, height=h, intr=INTR, pose=frames[2][1])                                  # frame 2's view, the source's only frame
    with s.b() as Bv, s.b() as fresh:
        b0 = Bv.debug_voxels(s.box)
        with B.Fusion(VS, 0.1, 10.0, initial_capacity=1 << 16) as E, s.a() as A, s.a() as A2:
            first = E.render(cam)                                                                   # builds the cache of the empty volume: no bricks
            assert first["stats"]["hits"] == 0
            r0 = A.render(cam)
            E.merge(Bv, pose); A.merge(Bv, pose); A2.merge(Bv, pose)
            if path == "aligned":
                seen = E.render(cam)
                assert seen["stats"]["hits"] > 500                                                  # sees the new voxels: the cache was dropped
            same_render(A.render(cam), A2.render(cam))                                             # equals the handle that never rendered before
            assert r0["stats"]["hits"] > 500
        b1 = Bv.debug_voxels(s.box)
        for k in ("found",) + FIELDS:
            assert np.array_equal(b0[k], b1[k]), k
        a, c = Bv.export(), fresh.export()                                                          # finish after having been merged from
        for k in ("keys", "sdf", "weight", "color"):
            assert np.array_equal(a[k], c[k]), k
        with B.Fusion(VS, 0.1, 10.0, initial_capacity=1 << 16) as E:                                # a finished source is read as it stands
            st = E.merge(Bv, pose)
            assert st["source_voxels"] == len(a["sdf"]) and st["sampled"] == st["allocated"] > 1000


# ---- 7. errors --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_errors(scenes):
    s = scenes["overlapping"]
    L = B.load(); p = B._p
    nan = np.array([0.0, 0.0, 0.0, np.nan, 0.0, 0.0]); inf = np.array([0.0, np.inf, 0.0, 0.0, 0.0, 0.0])
    st = B.MergeStats(); st.sampled = 77
    def unchanged(f, call, code, word):
        before = f.debug_voxels(s.box); info = f.info()
        assert call() == code and word in L.i3d_fusion_last_error(f.h).decode(), (code, L.i3d_fusion_last_error(f.h).decode())
        after = f.debug_voxels(s.box)
        assert all(np.array_equal(before[k], after[k]) for k in ("found",) + FIELDS) and f.info() == info and st.sampled == 77

    with s.a() as A, s.b() as Bv, B.Fusion(VS2, 0.1, 10.0) as other:
        assert L.i3d_fusion_merge(None, Bv.h, None, None) == 1
        unchanged(A, lambda: L.i3d_fusion_merge(A.h, None, None, C.byref(st)), 1, "null source")
        unchanged(A, lambda: L.i3d_fusion_merge(A.h, A.h, None, C.byref(st)), 1, "into itself")
        unchanged(A, lambda: L.i3d_fusion_merge(A.h, other.h, None, C.byref(st)), 1, "voxel size")
        unchanged(A, lambda: L.i3d_fusion_merge(A.h, Bv.h, p(nan), C.byref(st)), 1, "not finite")
        unchanged(A, lambda: L.i3d_fusion_merge(A.h, Bv.h, p(inf), C.byref(st)), 1, "not finite")
        try:
            far = B.Fusion(VS, 0.1, 10.0, device=1)                                                # only where the machine has a second device
        except B.I3DError:
            far = None
        if far is not None:
            with far:
                unchanged(A, lambda: L.i3d_fusion_merge(A.h, far.h, None, C.byref(st)), 1, "different devices")
        # an empty source: I3D_OK, zero counts, the ordinal consumed, the table untouched — and that ordinal is not a frame
        with B.Fusion(VS, 0.1, 10.0) as empty:
            before = A.debug_voxels(s.box)
            got = A.merge(empty, POSE)
            assert (got["ordinal"], got["source_voxels"], got["sampled"], got["allocated"], got["aligned"]) == (2, 0, 0, 0, 0) and A.info()["frames"] == 3
            after = A.debug_voxels(s.box)
            assert all(np.array_equal(before[k], after[k]) for k in ("found",) + FIELDS)
        with pytest.raises(B.I3DError):
            A.deintegrate(2, s.frames[2][0], s.frames[2][1], s.frames[2][2], s.frames[2][1], s.frames[2][3], 2)
        assert A.merge(Bv)["ordinal"] == 3                                                          # the handle goes on working
        assert A.finish(0) > 1000
        unchanged(A, lambda: L.i3d_fusion_merge(A.h, Bv.h, None, C.byref(st)), 4, "finished")       # integrate's rule and wording
        with pytest.raises(B.I3DError):
            A.merge(Bv)
        with pytest.raises(ValueError):
            Bv.merge(None)
