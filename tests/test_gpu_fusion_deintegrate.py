"""-m gpu: i3d_fusion_deintegrate / i3d_fusion_reintegrate on the device against their numpy statement (fusion_deintegrate_twin.py) and
the CPU oracle's Fusion: the shared contribution function is integrate's, a removal is the twin's bit for bit and the volume of the remaining frames within the
bounds of section 23.3, the fused call is the two calls it replaces bit for bit, an emptied volume is reusable, the correction loop the calls are for, the state
rules and errors, and app_fusion's repose_passes.

Two counts of the removal tests cannot hold for the LAST frame and are asserted for the first and the middle one only: no voxel can have a first frame after the
last ordinal, and a voxel only the last frame fed has no later frame to keep it valid."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fusion_cases as FC
import fusion_deintegrate_twin as DT
import helpers
import track_cases as TC
import track_twin
from fusion_cases import fusion_frames  # noqa: F401  (fixtures)
from intrinsic3d_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

VS = FC.VS
FIELDS = ("sdf", "weight", "color")


class Scene:
    """frames = [(depth, intr, bgr, c2w, erode)], and the oracle's raw volumes, each computed once: nat[i] after frames 0..i, rest(b) without frame b"""

    def __init__(self, oracle, frames, vs, poses=None):
        self.oracle, self.frames, self.vs, self.poses = oracle, frames, vs, poses
        self.nat = self.states(range(len(frames)))
        self._rest = {}

    def states(self, order, extra=()):
        o = self.oracle.Fusion(self.vs, 0.1, 10.0)
        out = []
        for fr in [self.frames[i] for i in order] + list(extra):
            d, intr, bgr, T, er = fr
            o.integrate(d, intr, bgr, intr, T, er)
            out.append(o.export())
        return out

    def rest(self, b):
        if b not in self._rest:
            self._rest[b] = self.states([i for i in range(len(self.frames)) if i != b])[-1]
        return self._rest[b]

    def fused(self, capacity=1 << 16, poses=None):
        f = B.Fusion(self.vs, 0.1, 10.0, initial_capacity=capacity)
        for i, (d, intr, bgr, T, er) in enumerate(self.frames):
            assert f.integrate(d, intr, bgr, intr, T if poses is None else poses[i], er) == i
        return f


def _args(fr, pose=None):
    d, intr, bgr, T, er = fr
    return (d, intr, bgr, intr, T if pose is None else pose, er)


@pytest.fixture(scope="module")
def scenes(oracle, fusion_frames):
    _, frames, _ = fusion_frames
    intr = FC.INTR.astype(np.float32)
    over = Scene(oracle, [(d, intr, FC.BGR, helpers.c2w(p), 2) for d, p in frames], VS, [p for _, p in frames])
    sc, fr = FC.textured_frames(seed=5, K=3, radius=10, w=96, h=72)
    ti = sc["intr"].astype(np.float32)
    tex = Scene(oracle, [(d, ti, bgr, T, 2) for d, bgr, T in fr], float(sc["voxel_size"]))
    return dict(overlapping=over, textured=tex)


def _same_state(a, b, sel=slice(None)):
    for k in FIELDS:
        assert np.array_equal(a[k][sel], b[k][sel]), (k, int((a[k][sel] != b[k][sel]).sum()))


# ---- 1. the samples are the integrate's ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["overlapping", "textured"])
def test_samples_are_the_integrates(scenes, name):
    s = scenes[name]
    empty = dict(keys=np.zeros((0, 3), np.int32), sdf=np.zeros(0, np.float32), weight=np.zeros(0, np.float32), color=np.zeros((0, 3), np.uint8))
    fed = 0
    with B.Fusion(s.vs, 0.1, 10.0, initial_capacity=1 << 10) as f:
        for i, fr in enumerate(s.frames):
            keys = s.nat[i]["keys"]
            smp = f.debug_frame_samples(keys, *_args(fr))                       # taken before the frame: the function reads no table
            want = DT.lookup(s.nat[i], keys)
            assert want["found"].all()
            _same_state(DT.integrate(DT.lookup(s.nat[i - 1] if i else empty, keys), smp), want)
            assert np.all(smp["wu"][smp["on"]] >= 3.0) and not smp["wu"][~smp["on"]].any() and not smp["has_color"][~smp["on"]].any()
            fed += int(smp["on"].sum())
            assert f.integrate(*_args(fr)) == i
            got = f.debug_voxels(keys)
            assert got["found"].all()
            _same_state(got, want)
            assert np.array_equal(got["first_frame"], DT.first_frames(s.nat[:i + 1], keys))
            away = keys + np.array([4000, 0, 0], np.int32)                          # keys that are not stored
            miss = f.debug_voxels(away[:65])
            assert not miss["found"].any() and np.all(miss["first_frame"] == -1) and not miss["weight"].any()
    assert fed > 3000


# ---- 2. / 3. a removal: the twin's bit for bit, the volume of the remaining frames within the bounds -------------------------------------------------------
REMOVALS = [("overlapping", 0), ("overlapping", 1), ("overlapping", 3), ("textured", 1)]


@pytest.fixture(scope="module")
def removals(scenes):
    made = {}

    def get(name, b):
        if (name, b) not in made:
            s = scenes[name]
            keys = s.nat[-1]["keys"]
            with s.fused() as f:
                before = f.debug_voxels(keys)
                smp = f.debug_frame_samples(keys, *_args(s.frames[b]))
                f.deintegrate(b, *_args(s.frames[b]))
                after = f.debug_voxels(keys)
                info = f.info()
            made[(name, b)] = dict(keys=keys, before=before, smp=smp, after=after, info=info)
        return made[(name, b)]
    return get


@pytest.mark.parametrize("name,b", REMOVALS)
def test_removal_is_the_twins_bit_for_bit(scenes, removals, name, b):
    s, r = scenes[name], removals(name, b)
    before, smp, after = r["before"], r["smp"], r["after"]
    assert before["found"].all() and after["found"].all() and np.array_equal(before["first_frame"], after["first_frame"])
    assert r["info"]["frames"] == len(s.frames)                                  # frames counts integrate operations
    _same_state(after, DT.deintegrate(before, smp, before["first_frame"], b))
    sel = smp["on"] & (before["first_frame"] <= b)
    _same_state(after, before, ~sel)                                             # voxels not selected are bitwise unchanged
    assert sel.sum() > 1000
    protected = int((smp["on"] & (before["first_frame"] > b)).sum())
    rest = s.rest(b)
    absent = int(((after["weight"] > 0) & ~DT.lookup(rest, r["keys"])["found"]).sum())
    print(f"{name}, frame {b} out: {int(sel.sum())} voxels fed, {int((sel & (after['weight'] == 0)).sum())} reset, {protected} protected by the first-frame rule, "
          f"{absent} valid voxels absent from the volume of the remaining frames")
    if name == "overlapping" and b < len(s.frames) - 1:
        assert protected >= 20 and absent >= 5


@pytest.mark.parametrize("name,b", REMOVALS)
def test_removal_against_never_integrated(scenes, removals, name, b):
    s, r = scenes[name], removals(name, b)
    rest = s.rest(b)
    valid = rest["weight"] > 0                                                   # every valid voxel of the remaining frames' volume, none left out
    at = lambda st: DT.lookup(dict(keys=r["keys"], **{f: st[f] for f in FIELDS}), rest["keys"][valid])  # noqa: E731
    got, before = at(r["after"]), at(r["before"])
    assert got["found"].all() and np.all(got["weight"] > 0)
    smp_at = DT.lookup(dict(keys=r["keys"], sdf=np.where(r["smp"]["on"] & (r["before"]["first_frame"] <= b), r["smp"]["sample"], np.float32(0)),
                            weight=r["before"]["weight"], color=r["before"]["color"]), rest["keys"][valid])["sdf"]
    bd = DT.bounds(before, got, smp_at, len(s.frames))
    e = dict(sdf=np.abs(got["sdf"].astype(np.float64) - rest["sdf"][valid]), weight=np.abs(got["weight"].astype(np.float64) - rest["weight"][valid]),
             color=np.abs(got["color"].astype(np.float64) - rest["color"][valid]).max(1))
    ratio = {k: float(np.max(np.where(bd[k] > 0, e[k] / np.where(bd[k] > 0, bd[k], 1.0), np.where(e[k] > 0, np.inf, 0.0)))) for k in e}
    print(f"{name}, frame {b} out against never integrated, {int(valid.sum())} voxels: largest error / bound {ratio}")
    assert ratio["sdf"] <= 1.0 and ratio["weight"] <= 1.0 and ratio["color"] <= 1.0, ratio


# ---- 4. the fused call is the two calls it replaces ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moved(scenes):
    """frame 1 of the overlapping scene moved to a perturbed pose by the fused call and by the two calls it replaces, then moved back by the fused call"""
    s = scenes["overlapping"]
    b = 1
    fr = s.frames[b]
    new_pose = helpers.c2w(track_twin.perturb(s.poses[b], np.random.default_rng(7), 0.5, 1.0 * VS))
    keys = s.states(range(len(s.frames)), extra=[(fr[0], fr[1], fr[2], new_pose, fr[4])])[-1]["keys"]      # the table's keys after the move: allocation is the oracle's
    r = dict(b=b, keys=keys)
    with s.fused(1 << 10) as one, s.fused(1 << 10) as two:                       # 4096 slots at first: the table grows between the calls
        r["start"] = one.debug_voxels(keys)
        r["smp_old"] = one.debug_frame_samples(keys, *_args(fr)); r["smp_new"] = one.debug_frame_samples(keys, *_args(fr, new_pose))
        r["n"] = one.reintegrate(b, *_args(fr)[:5], new_pose, fr[4])
        two.deintegrate(b, *_args(fr)); r["m"] = two.integrate(*_args(fr, new_pose))
        r["info"] = (one.info(), two.info())
        r["fused"], r["composed"] = one.debug_voxels(keys), two.debug_voxels(keys)
        r["back"] = one.reintegrate(r["n"], *_args(fr)[:4], new_pose, fr[3], fr[4])
        r["returned"] = one.debug_voxels(keys)
        with pytest.raises(B.I3DError):
            one.deintegrate(r["n"], *_args(fr, new_pose))                        # the ordinal left with the move
    return r


def test_reintegrate_equals_deintegrate_then_integrate(scenes, moved):
    s, r = scenes["overlapping"], moved
    a, c, n = r["fused"], r["composed"], r["n"]
    assert len(r["keys"]) > len(s.nat[-1]["keys"])
    assert n == r["m"] == len(s.frames) and r["info"][0] == r["info"][1] and r["info"][0]["frames"] == len(s.frames) + 1
    assert a["found"].all() and c["found"].all() and np.array_equal(a["first_frame"], c["first_frame"])
    _same_state(a, c)
    assert int((a["first_frame"] == n).sum()) == len(r["keys"]) - len(s.nat[-1]["keys"])
    _same_state(a, DT.reintegrate(r["start"], r["smp_old"], r["smp_new"], a["first_frame"], r["b"]))
    assert not np.array_equal(a["sdf"], r["start"]["sdf"])


def test_moved_and_moved_back(scenes, moved):
    """Every voxel valid before the two moves against what it held then.  A frame that is put in feeds every stored voxel its gates pass (23.1 item 2), so the
    move back also feeds the voxels a LATER frame first inserted - those the first-frame rule kept out of the removal, which the frame had never fed before: for
    them what they held then is the start state with the frame's sample added (the twin's integrate), for all others the start state itself.
    The bound is bound 3 (DT.bounds, the function the removal tests use), once per removal the voxel went through: the first move takes the frame out at the old
    pose (before = what the voxel held at the start, after = the twin's state with the frame out), the move back takes it out at the new pose (before = the state
    after the first move, after = the twin's state with the frame out again).  A voxel is held to the larger of the two; the ratio against the first alone is
    printed beside it.  n = the integrate operations before each removal."""
    s, r = scenes["overlapping"], moved
    start, a, z, smp_old, smp_new, b, n = r["start"], r["fused"], r["returned"], r["smp_old"], r["smp_new"], r["b"], r["n"]
    assert r["back"] == n + 1
    was = start["weight"] > 0
    assert z["found"].all() and np.all(z["weight"][was] > 0)
    late = smp_old["on"] & (a["first_frame"] > b) & start["found"]
    want = DT.integrate(start, smp_old, sel=late)
    assert 20 <= int((late & was).sum()) < 200
    first = a["first_frame"]
    fed_old = smp_old["on"] & (first <= b); fed_new = smp_new["on"]
    b1 = DT.bounds(want, DT.deintegrate(start, smp_old, first, b), np.where(fed_old, smp_old["sample"], np.float32(0)), n)
    b2 = DT.bounds(a, DT.deintegrate(a, smp_new, first, n), np.where(fed_new, smp_new["sample"], np.float32(0)), n + 1)
    e = dict(sdf=np.abs(z["sdf"].astype(np.float64) - want["sdf"]), weight=np.abs(z["weight"].astype(np.float64) - want["weight"]),
             color=np.abs(z["color"].astype(np.float64) - want["color"]).max(1))

    def ratio(bd, k):
        return float(np.max(np.where(bd[k][was] > 0, e[k][was] / np.where(bd[k][was] > 0, bd[k][was], 1.0), np.where(e[k][was] > 0, np.inf, 0.0))))
    both = {k: np.maximum(b1[k], b2[k]) for k in e}
    print(f"moved and moved back, {int(was.sum())} voxels ({int((late & was).sum())} fed for the first time on the way back): largest error / bound "
          f"{ {k: round(ratio(both, k), 3) for k in e} }; against the first removal's bound alone { {k: round(ratio(b1, k), 3) for k in e} }")
    assert all(ratio(both, k) <= 1.0 for k in e)


# ---- 5. empty and reuse -------------------------------------------------------------------------------------------------------------------------------------------
def test_emptied_volume_and_reuse(scenes):
    s = scenes["textured"]
    with s.fused() as f:
        for i in (1, 0, 2):
            f.deintegrate(i, *_args(s.frames[i]))
        got = f.debug_voxels(s.nat[-1]["keys"])
        assert got["found"].all() and not got["weight"].any() and not got["sdf"].any() and not got["color"].any()
        assert f.finish(0) == 0 and f.export()["keys"].shape == (0, 3)
    solo = s.states([1])[-1]
    with s.fused() as f:
        for i in (2, 1, 0):
            f.deintegrate(i, *_args(s.frames[i]))
        assert f.integrate(*_args(s.frames[1])) == 3
        got = f.debug_voxels(solo["keys"])
        assert got["found"].all() and (solo["weight"] > 0).sum() > 1000
        _same_state(got, solo)


# ---- 6. the loop it is for ------------------------------------------------------------------------------------------------------------------------------------------
def test_take_out_register_put_back(scenes, fusion_frames):
    scene = fusion_frames[0]
    s = scenes["overlapping"]
    depth, truth = s.frames[1][0], s.poses[1]
    wrong = track_twin.perturb(truth, np.random.default_rng(3), 0.5, 1.0 * VS)
    poses = [fr[3] for fr in s.frames]; poses[1] = helpers.c2w(wrong)
    with s.fused(poses=poses) as f:
        f.deintegrate(1, *_args(s.frames[1], poses[1]))
        pose, st = f.track_sdf(depth, wrong, FC.INTR)                           # against the other three frames
        s_err, e_err = TC.centre_in_camera(scene, wrong, truth, VS), TC.centre_in_camera(scene, pose, truth, VS)
        print(f"frame 1 taken out and registered against the rest: {st}, the sphere's centre in the camera frame {s_err:.3f} -> {e_err:.3f} voxel off")
        assert st["status"] in (0, 1) and st["inliers"] > 500
        assert s_err > 0.5 and e_err < 0.5 * s_err and st["rms_final"] < st["rms_initial"]
        new = f.integrate(*_args(s.frames[1], helpers.c2w(pose)))
        assert new == 4
        # the same correction as one move of the frame still in the volume, from the pose just found
        with s.fused(poses=poses) as g:
            assert g.reintegrate(1, *_args(s.frames[1])[:4], poses[1], helpers.c2w(pose), 2) == 4
            keys = s.nat[-1]["keys"]
            a, c = f.debug_voxels(keys), g.debug_voxels(keys)
            _same_state(a, c)
            assert np.array_equal(a["first_frame"], c["first_frame"])


# ---- 7. state and errors ------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_and_errors(scenes):
    s = scenes["overlapping"]
    L = B.load(); p = B._p
    keys = s.nat[-1]["keys"]
    d, intr, bgr, T, er = s.frames[0]
    h, w = d.shape

    def raw(f, name, ordinal, depth=d, pose=T, tail=()):
        fn = getattr(L, name)
        return fn(f.h, ordinal, w, h, p(intr), w, h, p(intr), p(depth), p(bgr), p(pose), er, *tail)

    def unchanged(f, call, code, word):
        before = f.debug_voxels(keys); info = f.info()
        assert call() == code and word in L.i3d_fusion_last_error(f.h).decode(), (code, L.i3d_fusion_last_error(f.h).decode())
        after = f.debug_voxels(keys)
        _same_state(before, after)
        assert np.array_equal(before["first_frame"], after["first_frame"]) and f.info() == info
    new = C.c_uint64(77)
    move = (p(T), C.byref(new))
    with s.fused() as f:
        unchanged(f, lambda: raw(f, "i3d_fusion_deintegrate", 4), 4, "ordinal 4")                   # never integrated
        unchanged(f, lambda: raw(f, "i3d_fusion_reintegrate", 99, tail=move), 4, "ordinal 99")
        unchanged(f, lambda: raw(f, "i3d_fusion_deintegrate", 0, depth=None), 1, "bad arguments")   # as integrate's
        unchanged(f, lambda: raw(f, "i3d_fusion_deintegrate", 0, pose=None), 1, "bad arguments")
        unchanged(f, lambda: raw(f, "i3d_fusion_reintegrate", 0, tail=(None, C.byref(new))), 1, "bad arguments")
        unchanged(f, lambda: L.i3d_fusion_deintegrate(f.h, 0, 0, h, p(intr), w, h, p(intr), p(d), p(bgr), p(T), er), 1, "bad arguments")
        assert new.value == 77
        assert raw(f, "i3d_fusion_deintegrate", 0) == 0
        unchanged(f, lambda: raw(f, "i3d_fusion_deintegrate", 0), 4, "already taken out")            # the same ordinal twice
        unchanged(f, lambda: raw(f, "i3d_fusion_reintegrate", 0, tail=move), 4, "already taken out")
        assert L.i3d_fusion_debug_voxels(f.h, -1, p(keys), None, None, None, None, None) == 1 and L.i3d_fusion_debug_voxels(f.h, 0, None, None, None, None, None, None) == 0
        assert L.i3d_fusion_debug_voxels(f.h, 4, p(keys), None, None, None, None, None) == 1
        assert f.finish(0) > 1000
        fin = f.debug_voxels(keys)                                                                   # the lookups still read a finished volume
        assert fin["found"].all()
        for call in (lambda: raw(f, "i3d_fusion_deintegrate", 1), lambda: raw(f, "i3d_fusion_reintegrate", 1, tail=move)):
            assert call() == 4 and "finished" in L.i3d_fusion_last_error(f.h).decode()
        _same_state(fin, f.debug_voxels(keys))
        with pytest.raises(B.I3DError):
            f.deintegrate(2, d, intr, bgr, intr, T, er)
    # the renderer follows: no hits once the only frame is out; in, out and in again is the single integrate (every voxel the frame fed was reset to Voxel(), so
    # the bound's quotient is 1: 8 eps of the truncation in sdf, which the unit-slope field turns into depth one to one)
    cam = dict(width=w, height=h, intr=FC.INTR, pose=s.poses[0])
    with B.Fusion(VS, 0.1, 10.0) as f, B.Fusion(VS, 0.1, 10.0) as g:
        assert f.integrate(*_args(s.frames[0])) == 0
        assert f.render(cam)["stats"]["hits"] > 500
        f.deintegrate(0, *_args(s.frames[0]))
        gone = f.render(cam)
        assert gone["stats"]["hits"] == 0 and not gone["depth"].any()
        assert f.integrate(*_args(s.frames[0])) == 1
        g.integrate(*_args(s.frames[0]))
        a, c = f.render(cam), g.render(cam)
        assert a["stats"]["hits"] == c["stats"]["hits"] > 500 and np.array_equal(a["depth"] > 0, c["depth"] > 0)
        gap = float(np.abs(a["depth"] - c["depth"]).max())
        print(f"in, out and in again against one integrate: largest depth difference {gap:.3e} m")
        assert gap <= 8.0 * DT.EPS * 5.0 * VS


# ---- 8. app_fusion ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_app_fusion_repose_passes(scenes, tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_dataset
    app = os.path.join(ROOT, "apps", "app_fusion")
    assert os.path.exists(app), "apps/app_fusion has not been built (run __graft_entry__.build())"
    s = scenes["overlapping"]
    sc = dict(voxel_size=VS, intr=FC.INTR, keys=np.zeros((1, 3), np.int32), sdf=np.zeros(1, np.float32), weight=np.ones(1, np.float32), color=np.zeros((1, 3), np.uint8),
              frames=[dict(depth=[fr[0]], bgr=[fr[2]]) for fr in s.frames], poses=s.poses)
    tracked = 'track_frames: "1"\ntrack_mode: "sdf"\n'
    vols = {}
    for name, extra in (("without", tracked), ("zero", tracked + 'repose_passes: "0"\n'), ("one", tracked + 'repose_passes: "1"\n')):
        out = tmp_path / name
        yml, _ = make_dataset.write_dataset(str(out), sc)
        with open(out / "fusion.yml", "a") as fh:
            fh.write(extra)
        r = subprocess.run([app, "-s", yml, "-f", str(out / "fusion.yml")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("repose pass 1" in r.stdout) == (name == "one"), r.stdout
        vols[name] = (out / "fusion" / f"volume_{VS:g}.tsdf").read_bytes()
    assert vols["without"] == vols["zero"] and len(vols["one"]) > 100000 and vols["one"] != vols["zero"]
    vol = B.tsdf_read(str(tmp_path / "one" / "fusion" / f"volume_{VS:g}.tsdf"))
    assert len(vol["sdf"]) > 3000 and np.isfinite(vol["sdf"]).all() and np.all(vol["weight"] > 0)
    out = tmp_path / "alone"
    yml, _ = make_dataset.write_dataset(str(out), sc)
    with open(out / "fusion.yml", "a") as fh:
        fh.write('repose_passes: "1"\n')
    r = subprocess.run([app, "-s", yml, "-f", str(out / "fusion.yml")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "repose_passes" in r.stderr
