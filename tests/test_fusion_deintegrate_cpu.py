"""-m "not gpu": the definition of i3d_fusion_deintegrate on the CPU oracle's Fusion and its numpy statement (fusion_deintegrate_twin.py).
A frame's contribution is measured from the oracle's states either side of the frame (weight difference; the sample from the weighted sums in fp64), the twin takes it
out of the volume of all frames, and the result is held against the oracle's volume of the remaining frames - with the first-frame rule, and, to show that the scene
needs it, without."""

import numpy as np
import pytest

import fusion_cases as FC
import fusion_deintegrate_twin as DT
import helpers
from fusion_cases import fusion_frames  # noqa: F401  (fixtures)

VS = FC.VS


def _overlapping(fusion_frames):
    _, frames, _ = fusion_frames
    intr = FC.INTR.astype(np.float32)
    return [(d, intr, FC.BGR, helpers.c2w(p), 2) for d, p in frames], VS


def _textured():
    sc, frames = FC.textured_frames(seed=5, K=3, radius=10, w=96, h=72)
    intr = sc["intr"].astype(np.float32)
    return [(d, intr, bgr, T, 2) for d, bgr, T in frames], float(sc["voxel_size"])


def _oracle_states(oracle, vs, frames, order):
    """raw exports of the oracle's volume after each frame of `order`"""
    o = oracle.Fusion(vs, 0.1, 10.0)
    out = []
    for i in order:
        d, intr, bgr, T, er = frames[i]
        o.integrate(d, intr, bgr, intr, T, er)
        out.append(o.export())
    return out


def _contribution(before, after, keys):
    """the frame between two states at `keys`: on = the weight changed; wu and the samples from the weighted sums either side, in fp64"""
    a, b = DT.lookup(after, keys), DT.lookup(before, keys)
    wa, wb = a["weight"].astype(np.float64), b["weight"].astype(np.float64)
    on = wa != wb
    wu = np.where(on, wa - wb, 1.0)
    sample = np.where(on, (a["sdf"].astype(np.float64) * wa - b["sdf"].astype(np.float64) * wb) / wu, 0.0)
    rgb = np.where(on[:, None], (a["color"].astype(np.float64) * wa[:, None] - b["color"].astype(np.float64) * wb[:, None]) / wu[:, None], 0.0)
    return dict(on=on, sample=sample.astype(np.float32), wu=np.where(on, wu, 0.0).astype(np.float32), has_color=on.copy(),
                rgb=np.clip(np.rint(rgb), 0, 255).astype(np.uint8))


def _remove(oracle, frames, vs, b):
    """everything the checks need for taking frame b out of the volume of all frames"""
    n = len(frames)
    others = [i for i in range(n) if i != b]
    nat = _oracle_states(oracle, vs, frames, range(n))                 # the natural order: the states either side of b, the first frames, the volume to take b out of
    last = _oracle_states(oracle, vs, frames, others + [b])            # b fused last: its gates over every voxel of the volume, the protected ones included
    rest = last[-2]                                                    # the volume that never saw b
    keys = nat[-1]["keys"]
    assert set(DT.pack(keys).tolist()) == set(DT.pack(last[-1]["keys"]).tolist())
    first = DT.first_frames(nat, keys)
    empty = dict(keys=np.zeros((0, 3), np.int32), sdf=np.zeros(0, np.float32), weight=np.zeros(0, np.float32), color=np.zeros((0, 3), np.uint8))
    smp = _contribution(nat[b - 1] if b > 0 else empty, nat[b], keys)  # exact where it matters: the voxels b fed
    gates = _contribution(last[-2], last[-1], keys)                    # b's gates over all voxels
    assert np.array_equal(gates["on"] & (first <= b), smp["on"])       # a frame feeds exactly the voxels that exist when it is fused and pass its gates
    protected = gates["on"] & (first > b)
    for k in ("sample", "wu", "rgb"):
        smp[k] = np.where(protected if smp[k].ndim == 1 else protected[:, None], gates[k], smp[k])
    smp["on"] = gates["on"]; smp["has_color"] = gates["on"].copy()
    state = DT.lookup(nat[-1], keys)
    return dict(keys=keys, first=first, smp=smp, state=state, rest=rest, protected=protected, n=n)


def _against_rest(r, got):
    """every valid voxel of the volume of the remaining frames: present, valid and within the bounds of section 23.3; returns the largest error-to-bound ratios.
    The colour sample is known only to a level here (it is recovered from truncated colours), which the removal amplifies by wu / w_after: that term is added to
    the colour bound of THIS check; the device test has the exact samples and holds the bound as it stands."""
    rest = r["rest"]
    valid = rest["weight"] > 0
    at = DT.lookup(dict(keys=r["keys"], **{k: got[k] for k in ("sdf", "weight", "color")}), rest["keys"][valid])
    if not (at["found"].all() and (at["weight"] > 0).all()):
        return None
    pos = DT.lookup(dict(keys=r["keys"], sdf=np.arange(len(r["keys"]), dtype=np.float32), weight=np.ones(len(r["keys"]), np.float32),
                         color=np.zeros((len(r["keys"]), 3), np.uint8)), rest["keys"][valid])["sdf"].astype(np.int64)
    before = {k: r["state"][k][pos] for k in ("sdf", "weight", "color")}
    on = r["smp"]["on"][pos] & (r["first"][pos] <= r["b"])
    bd = DT.bounds(before, at, np.where(on, r["smp"]["sample"][pos], 0.0), r["n"])
    wu = np.where(on, r["smp"]["wu"][pos], 0.0).astype(np.float64)
    bd["color"] = bd["color"] + wu / at["weight"].astype(np.float64)
    e = dict(sdf=np.abs(at["sdf"].astype(np.float64) - rest["sdf"][valid]), weight=np.abs(at["weight"].astype(np.float64) - rest["weight"][valid]),
             color=np.abs(at["color"].astype(np.float64) - rest["color"][valid]).max(1))
    ratios = {}
    for k in e:
        nz = bd[k] > 0
        assert np.all(e[k][~nz] == 0), k
        ratios[k] = float((e[k][nz] / bd[k][nz]).max()) if nz.any() else 0.0
    return ratios


@pytest.mark.parametrize("scene,b", [("overlapping", 1), ("overlapping", 0), ("textured", 1), ("textured", 0)])
def test_removal_reproduces_the_volume_of_the_remaining_frames(oracle, fusion_frames, scene, b):
    frames, vs = _overlapping(fusion_frames) if scene == "overlapping" else _textured()
    r = _remove(oracle, frames, vs, b); r["b"] = b
    got = DT.deintegrate(r["state"], r["smp"], r["first"], b)
    ratios = _against_rest(r, got)
    assert ratios is not None, "a valid voxel of the remaining frames is missing or invalid after the removal"
    fed = r["smp"]["on"] & (r["first"] <= b)
    reset = fed & (got["weight"] == 0)
    extra = int((got["weight"] > 0).sum() - (r["rest"]["weight"] > 0).sum())
    print(f"{scene}, frame {b} out: {len(r['keys'])} voxels, {int(fed.sum())} fed by the frame, {int(reset.sum())} reset, {int(r['protected'].sum())} protected by the "
          f"first-frame rule, {extra} valid voxels the remaining frames never allocate; largest error / bound: {ratios}")
    assert ratios["sdf"] <= 1.0 and ratios["weight"] <= 1.0 and ratios["color"] <= 1.0, ratios
    # the reset rule gives exactly Voxel(): a voxel only this frame fed has weight wu - wu = 0
    only = fed & (r["state"]["weight"] == r["smp"]["wu"])
    assert only.sum() > 0 and np.all(reset[only])
    assert not got["sdf"][reset].any() and not got["weight"][reset].any() and not got["color"][reset].any()
    assert np.all(got["weight"][fed & ~reset] >= 0.5)
    # voxels the frame did not feed are untouched
    for k in ("sdf", "weight", "color"):
        assert np.array_equal(got[k][~fed], r["state"][k][~fed]), k
    if scene == "overlapping":
        # the scene exercises the first-frame rule: without it the removal takes from voxels what the frame never gave them
        assert r["protected"].sum() >= 20
        naive = DT.deintegrate(r["state"], r["smp"], r["first"], b, first_frame_rule=False)
        rn = _against_rest(dict(r, first=np.zeros_like(r["first"])), naive)
        assert rn is None or max(rn["sdf"], rn["weight"]) > 1.0, rn


def test_reintegrate_is_deintegrate_then_integrate():
    rng = np.random.default_rng(0)
    n = 4096
    state = dict(sdf=rng.normal(0, 0.02, n).astype(np.float32), weight=rng.uniform(3, 40, n).astype(np.float32), color=rng.integers(0, 256, (n, 3)).astype(np.uint8))

    def smp():
        return dict(on=rng.random(n) < 0.6, sample=rng.normal(0, 0.02, n).astype(np.float32), wu=rng.uniform(3, 12, n).astype(np.float32),
                    has_color=rng.random(n) < 0.9, rgb=rng.integers(0, 256, (n, 3)).astype(np.uint8))
    a, b = smp(), smp()
    first = rng.integers(0, 4, n)
    state["weight"][:64] = a["wu"][:64]; a["on"][:64] = True; first[:64] = 0          # voxels only the leaving frame fed
    one = DT.reintegrate(state, a, b, first, 2)
    mid = DT.deintegrate(state, a, first, 2)
    two = DT.integrate(mid, b)
    for k in one:
        assert np.array_equal(one[k], two[k]), k
    assert not mid["weight"][:64].any() and not mid["sdf"][:64].any() and not mid["color"][:64].any()
    assert np.array_equal(two["weight"][:64][b["on"][:64]], b["wu"][:64][b["on"][:64]])
    sel = a["on"] & (first > 2)
    assert sel.sum() > 100 and all(np.array_equal(mid[k][sel], state[k][sel]) for k in mid)


def test_new_symbols_on_a_null_handle():
    from intrinsic3d_amd import binding as B
    L = B.load()
    z = np.zeros(64, np.float32); p = B._p
    assert L.i3d_fusion_deintegrate(None, 0, 4, 4, p(z), 4, 4, p(z), p(z), p(z), p(z), 0) == 1
    assert L.i3d_fusion_reintegrate(None, 0, 4, 4, p(z), 4, 4, p(z), p(z), p(z), p(z), 0, p(z), None) == 1
    assert L.i3d_fusion_debug_voxels(None, 1, p(z), p(z), p(z), p(z), p(z), p(z)) == 1
    assert L.i3d_fusion_debug_frame_samples(None, 4, 4, p(z), 4, 4, p(z), p(z), p(z), p(z), 0, 1, p(z), p(z), p(z), p(z), p(z), p(z)) == 1
