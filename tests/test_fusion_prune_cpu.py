"""No device: the surface of i3d_fusion_prune in the header, the ABI table, the binding and the library, and the self-checks of its numpy
statement (fusion_prune_twin.py) on hand-made volumes of a few dozen voxels: each criterion against a plain Python loop, a voxel failing two criteria, mode 2 as
the complement of mode 1, and the three boundary cases."""
import ctypes
import os
import re
import struct

import numpy as np

import fusion_load_twin as LT
import fusion_merge_twin as MT
import fusion_prune_twin as PT
from intrinsic3d_amd import abi, binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
VS = 0.0078125                                       # 2^-7: key * VS is exact, so a coordinate can lie exactly on a box face


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "intrinsic3d_hip.h")).read(), flags=re.S)


def test_the_symbol_is_declared_bound_and_exported():
    declared = re.findall(r"\b(i3d_[a-z0-9_]+)\s*\(", _header())
    table = [name for name, _, _ in abi.PROTOTYPES]
    lib = B.load()
    assert "i3d_fusion_prune" in declared
    assert table.count("i3d_fusion_prune") == 1 and "i3d_fusion_prune" in B.EXPORTS
    assert hasattr(lib, "i3d_fusion_prune")
    # directly after i3d_fusion_merge, in the header and in the table
    assert declared[declared.index("i3d_fusion_merge") + 1] == "i3d_fusion_prune"
    assert table[table.index("i3d_fusion_merge") + 1] == "i3d_fusion_prune"
    # the neighbourhoods other tests pin
    assert table.index("i3d_fusion_save") + 3 == table.index("i3d_fusion_snapshot") and table[table.index("i3d_cast_rays") + 1] == "i3d_fusion_cast_rays"
    proto = dict((n, (r, a)) for n, r, a in abi.PROTOTYPES)["i3d_fusion_prune"]
    assert proto[0] is abi.i32 and len(proto[1]) == 7 and proto[1][1] is abi.f32 and proto[1][2] is abi.f32
    assert callable(B.Fusion.prune)


def test_no_new_struct():
    declared = set(re.findall(r"\}\s*(i3d_[a-z0-9_]+)\s*;", _header())) - {"i3d_status", "i3d_lm_record"}
    mirrors = {v._c_name_ for v in vars(abi).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and "_c_name_" in vars(v)}
    assert len(declared) == 25 and declared == mirrors, sorted(declared ^ mirrors)


# ---- the twin on hand-made volumes -------------------------------------------------------------------------------------------------------------------------------
def _volume(n=48, seed=3):
    rng = np.random.default_rng(seed)
    k = rng.integers(-6, 7, (8 * n, 3)).astype(np.int64)
    _, first = np.unique(PT.pack(k), return_index=True)
    k = k[np.sort(first)][:n]
    assert len(k) == n
    w = rng.integers(0, 5, n).astype(F); w[::5] = 0.0
    s = (rng.uniform(-0.06, 0.06, n)).astype(F); s[w == 0] = 0.0
    return MT.volume(k, s, w, rng.integers(0, 256, (n, 3)), rng.integers(0, 3, n))


def _loop(vol, min_weight=0.0, max_abs_sdf=0.0, box=None, box_mode=None):
    """item 1 voxel by voxel; float32 through struct, so that no numpy comparison is shared with the twin"""
    def f32(x):
        return struct.unpack("f", struct.pack("f", float(x)))[0]
    mode = (0 if box is None else 1) if box_mode is None else box_mode
    out = []
    for (x, y, z), s, w in zip(vol["keys"].tolist(), vol["sdf"].tolist(), vol["weight"].tolist()):
        v = 0
        if f32(min_weight) >= 0 and not (w > f32(min_weight)):
            v |= 1
        if f32(max_abs_sdf) > 0 and abs(s) > f32(max_abs_sdf):
            v |= 2
        if mode:
            wc = [f32(f32(c) * f32(VS)) for c in (x, y, z)]
            b = [f32(q) for q in box]
            outside = wc[0] < b[0] or wc[0] > b[1] or wc[1] < b[2] or wc[1] > b[3] or wc[2] < b[4] or wc[2] > b[5]
            if outside == (mode == 1):
                v |= 4
        out.append(v)
    return np.array(out, np.uint8)


BOX = (-3 * VS, 2 * VS, -2 * VS, 4 * VS, -6 * VS, 1 * VS)
WIDE = (-5 * VS, 5 * VS, -5 * VS, 6 * VS, -6 * VS, 4 * VS)
CASES = (dict(), dict(min_weight=1.0), dict(min_weight=-1.0, max_abs_sdf=0.03), dict(min_weight=-1.0, box=BOX), dict(min_weight=-1.0, box=BOX, box_mode=2),
         dict(min_weight=0.0, max_abs_sdf=0.05, box=WIDE), dict(min_weight=-1.0))


def test_each_criterion_against_a_plain_loop():
    vol = _volume()
    seq = vol["keys"][np.random.default_rng(1).permutation(len(vol["keys"]))]
    for params in CASES:
        v = PT.verdict(vol["keys"], vol["sdf"], vol["weight"], VS, **params)
        want = _loop(vol, **params)
        assert np.array_equal(v, want), params
        out, seq_out, counts = PT.prune(vol, seq, voxel_size=VS, **params)
        assert counts == [len(v), int((want != 0).sum()), int((want & 1 != 0).sum()), int((want & 2 != 0).sum()), int((want & 4 != 0).sum())], params
        keep = want == 0
        for k in ("keys", "sdf", "weight", "color", "first_frame"):
            assert np.array_equal(out[k], vol[k][keep]), (params, k)
        assert np.array_equal(seq_out, seq[np.isin(PT.pack(seq), PT.pack(vol["keys"][keep]))]), params
        if params and params != dict(min_weight=-1.0):
            assert 0 < counts[1] < counts[0], params                       # every case but the last splits the volume
    assert PT.prune(vol, seq, voxel_size=VS, min_weight=-1.0)[2] == [48, 0, 0, 0, 0]
    d = PT.prune(vol, seq)[2]
    assert d[1] == d[2] == int((vol["weight"] == 0).sum()) > 0 and d[3] == d[4] == 0      # the defaults: exactly the weightless voxels


def test_both_volume_shapes_agree():
    vol = _volume(); seq = vol["keys"][::-1]
    by_key = LT.volume_of(vol["keys"], vol["sdf"], vol["weight"], vol["color"], vol["first_frame"])
    for params in CASES:
        a, sa, ca = PT.prune(vol, seq, voxel_size=VS, **params)
        b, sb, cb = PT.prune(by_key, seq, voxel_size=VS, **params)
        assert ca == cb and np.array_equal(sa, sb)
        assert b == LT.volume_of(a["keys"], a["sdf"], a["weight"], a["color"], a["first_frame"])


def test_a_voxel_failing_two_criteria_counts_in_each():
    vol = MT.volume([[0, 0, 0], [1, 0, 0], [2, 0, 0], [9, 0, 0]], [0.0, 0.05, 0.05, 0.0], [0.0, 0.0, 3.0, 3.0])
    box = (-VS, 3 * VS, -VS, VS, -VS, VS)
    out, seq, counts = PT.prune(vol, vol["keys"], voxel_size=VS, min_weight=0.0, max_abs_sdf=0.01, box=box)
    # voxel 0 fails W; 1 fails W and S; 2 fails S; 3 fails B: four removed, two W, two S, one B
    assert counts == [4, 4, 2, 2, 1] and len(out["keys"]) == 0 and len(seq) == 0
    assert list(PT.verdict(vol["keys"], vol["sdf"], vol["weight"], VS, min_weight=0.0, max_abs_sdf=0.01, box=box)) == [1, 3, 2, 4]


def test_mode_2_is_the_complement_of_mode_1():
    vol = _volume(n=60, seed=8)
    a = PT.verdict(vol["keys"], vol["sdf"], vol["weight"], VS, min_weight=-1.0, box=BOX, box_mode=1) != 0
    b = PT.verdict(vol["keys"], vol["sdf"], vol["weight"], VS, min_weight=-1.0, box=BOX, box_mode=2) != 0
    assert np.array_equal(a, ~b) and 0 < a.sum() < len(a)
    assert np.array_equal(PT.verdict(vol["keys"], vol["sdf"], vol["weight"], VS, min_weight=-1.0, box=BOX) != 0, a)      # a box alone means mode 1


def test_boundaries():
    k = [[0, 0, 0], [1, 0, 0], [2, 0, 0]]
    # w == min_weight fails (the test is w > min_weight); the next float above stays
    w = np.array([2.0, np.nextafter(F(2.0), F(3.0)), np.nextafter(F(2.0), F(1.0))], F)
    assert list(PT.verdict(k, np.zeros(3, F), w, VS, min_weight=2.0)) == [1, 0, 1]
    # |s| == max_abs_sdf stays (the test is |s| > max_abs_sdf), either sign
    m = F(0.03)
    s = np.array([m, -m, np.nextafter(m, F(1.0))], F)
    assert list(PT.verdict(k, s, np.ones(3, F), VS, min_weight=-1.0, max_abs_sdf=float(m))) == [0, 0, 2]
    # a coordinate exactly on a face is inside: kept by mode 1, erased by mode 2
    box = (0.0, 1 * VS, 0.0, 0.0, 0.0, 0.0)
    assert list(PT.verdict(k, np.zeros(3, F), np.ones(3, F), VS, min_weight=-1.0, box=box, box_mode=1)) == [0, 0, 4]
    assert list(PT.verdict(k, np.zeros(3, F), np.ones(3, F), VS, min_weight=-1.0, box=box, box_mode=2)) == [4, 4, 0]
    # max_abs_sdf = 0 and box_mode = 0 switch their criteria off; min_weight < 0 switches W off
    assert not PT.verdict(k, np.full(3, 9.0, F), np.zeros(3, F), VS, min_weight=-1.0, max_abs_sdf=0.0, box=box, box_mode=0).any()


def test_capacity_rule():
    assert PT.capacity_after(1 << 16, 100, 5, False) == 1 << 16 and PT.capacity_after(1 << 16, 100, 0, True) == 1 << 16
    assert PT.capacity_after(1 << 16, 0, 5, True) == 4096 and PT.capacity_after(1 << 16, 2048, 5, True) == 4096 and PT.capacity_after(1 << 16, 2049, 5, True) == 8192
    assert PT.capacity_after(4096, 2399, 1, True) == 4096                 # never above the current capacity
