"""No device: the surface of i3d_fusion_components / _get_components / _prune_components in the header, the ABI table, the binding and the
library, and the self-checks of the numpy statement (fusion_components_twin.py) against a plain Python flood fill on hand-made volumes of a few dozen voxels: the
tie rule, the three boundary cases of the node criteria, keys that touch by an edge or a corner only, and the removal rule with each of its switches."""
import os
import re

import numpy as np
import pytest

import fusion_components_twin as CT
import fusion_prune_twin as PT
from intrinsic3d_amd import abi, binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("i3d_fusion_components", "i3d_fusion_get_components", "i3d_fusion_prune_components")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "intrinsic3d_hip.h")).read(), flags=re.S)


def test_the_symbols_are_declared_bound_and_exported():
    declared = re.findall(r"\b(i3d_[a-z0-9_]+)\s*\(", _header())
    table = [name for name, _, _ in abi.PROTOTYPES]
    lib = B.load()
    for name in NAMES:
        assert declared.count(name) == 1 and table.count(name) == 1 and name in B.EXPORTS and hasattr(lib, name), name
    # directly after i3d_fusion_prune, in this order, in the header and in the table
    for names in (declared, table):
        at = names.index("i3d_fusion_prune")
        assert tuple(names[at + 1:at + 4]) == NAMES and names[at - 1] == "i3d_fusion_merge"
    proto = dict((n, (r, a)) for n, r, a in abi.PROTOTYPES)
    r, a = proto["i3d_fusion_components"]
    assert r is abi.i32 and len(a) == 4 and a[1] is abi.f32 and a[2] is abi.f32
    r, a = proto["i3d_fusion_get_components"]
    assert r is abi.i32 and len(a) == 4
    r, a = proto["i3d_fusion_prune_components"]
    assert r is abi.i32 and len(a) == 7 and a[1] is abi.f32 and a[2] is abi.f32 and a[3] is abi.i64 and a[4] is abi.i64 and a[5] is abi.i32
    assert callable(B.Fusion.components) and callable(B.Fusion.prune_components)


def test_still_25_structs():
    declared = set(re.findall(r"\}\s*(i3d_[a-z0-9_]+)\s*;", _header())) - {"i3d_status", "i3d_lm_record"}
    assert len(declared) == 25, sorted(declared)


# ---- the plain statement: a flood fill over a dict, one voxel at a time ---------------------------------------------------------------------------------------------
def _flood(keys, sdf, weight, min_weight=0.0, max_abs_sdf=0.0):
    """(sorted node keys, label, sizes) by a stack-based flood fill; every comparison in float32 as section 38.1 item 1 writes it"""
    def packed(k):
        return ((k[2] + (1 << 20)) << 42) | ((k[1] + (1 << 20)) << 21) | (k[0] + (1 << 20))
    node = []
    for k, s, w in zip(keys.tolist(), sdf, weight):
        ok = True
        if F(min_weight) >= F(0) and not (F(w) > F(min_weight)):
            ok = False
        if F(max_abs_sdf) > F(0) and abs(F(s)) > F(max_abs_sdf):
            ok = False
        if ok:
            node.append(tuple(k))
    node.sort(key=packed)
    index = {k: i for i, k in enumerate(node)}
    comp = [-1] * len(node); members = []
    for i, k in enumerate(node):
        if comp[i] >= 0:
            continue
        comp[i] = len(members); mine = [i]; stack = [k]
        while stack:
            x, y, z = stack.pop()
            for nb in ((x + 1, y, z), (x - 1, y, z), (x, y + 1, z), (x, y - 1, z), (x, y, z + 1), (x, y, z - 1)):
                j = index.get(nb)
                if j is not None and comp[j] < 0:
                    comp[j] = comp[i]; mine.append(j); stack.append(nb)
        members.append(mine)
    order = sorted(range(len(members)), key=lambda c: (-len(members[c]), min(members[c])))
    number = {c: r for r, c in enumerate(order)}
    return (np.array(node, np.int32).reshape(-1, 3), np.array([number[c] for c in comp], np.int32), np.array([len(members[c]) for c in order], np.int64))


def _vol(keys, sdf=None, weight=None):
    keys = np.asarray(keys, np.int32).reshape(-1, 3); n = len(keys)
    return dict(keys=keys, sdf=np.zeros(n, F) if sdf is None else np.asarray(sdf, F), weight=np.ones(n, F) if weight is None else np.asarray(weight, F),
                color=np.zeros((n, 3), np.uint8), first_frame=np.zeros(n, np.int64))


def _check(vol, **params):
    got = CT.components(vol, 0.01, **params)
    k, lab, sz = _flood(vol["keys"], vol["sdf"], vol["weight"], **params)
    assert np.array_equal(got["keys"], k) and np.array_equal(got["label"], lab) and np.array_equal(got["sizes"], sz), (got, k, lab, sz)
    assert got["nodes"] == len(k) and got["components"] == len(sz) and got["largest"] == (int(sz[0]) if len(sz) else 0)
    assert got["keys"].dtype == np.int32 and got["label"].dtype == np.int32 and got["sizes"].dtype == np.int64
    return got


def _run(x0, x1, y, z):
    return [(x, y, z) for x in range(x0, x1)]


def test_the_tie_rule_and_the_order():
    # two runs of 3 (the one with the smaller packed key - smaller z - comes first whatever its x), one of 5, two single voxels
    keys = _run(40, 43, 0, -2) + _run(-9, -6, 5, 3) + _run(0, 5, 1, 1) + [(7, 7, 7), (-7, -7, -7)]
    rng = np.random.default_rng(3)
    vol = _vol(np.array(keys)[rng.permutation(len(keys))])
    got = _check(vol)
    assert got["sizes"].tolist() == [5, 3, 3, 1, 1]
    by_key = {tuple(k): int(c) for k, c in zip(got["keys"].tolist(), got["label"])}
    assert by_key[(0, 1, 1)] == 0 and by_key[(40, 0, -2)] == 1 and by_key[(-9, 5, 3)] == 2 and by_key[(-7, -7, -7)] == 3 and by_key[(7, 7, 7)] == 4
    assert np.array_equal(PT.pack(got["keys"]), np.sort(PT.pack(got["keys"])))
    assert _check(_vol(np.zeros((0, 3))))["nodes"] == 0


def test_the_boundary_cases_of_the_criteria():
    keys = _run(0, 7, 0, 0)
    # w == min_weight is not a node: the run falls apart at x = 3
    w = np.full(7, 2.0, F); w[3] = 1.5
    assert _check(_vol(keys, weight=w), min_weight=1.5)["sizes"].tolist() == [3, 3]
    assert _check(_vol(keys, weight=w), min_weight=1.25)["sizes"].tolist() == [7]
    # |s| == max_abs_sdf is a node, the next float above is not; max_abs_sdf = 0 is off
    s = np.zeros(7, F); s[3] = -0.25
    assert _check(_vol(keys, sdf=s), max_abs_sdf=0.25)["sizes"].tolist() == [7]
    assert _check(_vol(keys, sdf=s), max_abs_sdf=float(np.nextafter(F(0.25), F(0))))["sizes"].tolist() == [3, 3]
    assert _check(_vol(keys, sdf=s))["sizes"].tolist() == [7]
    # a weightless voxel is no node by default, and one with a negative min_weight (W off)
    w = np.ones(7, F); w[2] = 0.0
    assert _check(_vol(keys, weight=w))["sizes"].tolist() == [4, 2]
    assert _check(_vol(keys, weight=w), min_weight=-1.0)["sizes"].tolist() == [7]
    assert CT.nodes(s, w).tolist() == [True, True, False, True, True, True, True]


def test_edges_and_corners_do_not_connect():
    assert _check(_vol([(0, 0, 0), (1, 1, 0)]))["sizes"].tolist() == [1, 1]              # an edge
    assert _check(_vol([(0, 0, 0), (1, 1, 1)]))["sizes"].tolist() == [1, 1]              # a corner
    assert _check(_vol([(0, 0, 0), (0, 1, 1), (1, 0, 1)]))["sizes"].tolist() == [1, 1, 1]
    assert _check(_vol([(0, 0, 0), (0, 1, 0), (0, 1, 1), (-1, 1, 1)]))["sizes"].tolist() == [4]
    assert _check(_vol([(5, 0, 0), (4, 1, 0)]))["sizes"].tolist() == [1, 1]              # neighbours in key order, not in space
    assert _check(_vol([(-1, 0, 0), (0, 0, 0)]))["sizes"].tolist() == [2]
    rng = np.random.default_rng(8)
    box = np.stack(np.meshgrid(*[np.arange(-3, 4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    for density in (0.2, 0.35, 0.6):
        got = _check(_vol(box[rng.random(len(box)) < density]))
        assert got["components"] > 1


@pytest.mark.parametrize("min_voxels,keep_largest,gone", [(0, 0, []), (3, 0, [3, 4]), (4, 0, [1, 2, 3, 4]), (0, 2, [2, 3, 4]), (3, 4, [3, 4]), (4, 4, [1, 2, 3, 4]),
                                                          (2, 1, [1, 2, 3, 4]), (100, 0, [0, 1, 2, 3, 4]), (0, 9, [])])
def test_the_removal_rule(min_voxels, keep_largest, gone):
    keys = _run(40, 43, 0, -2) + _run(-9, -6, 5, 3) + _run(0, 5, 1, 1) + [(7, 7, 7), (-7, -7, -7)] + [(20, 20, 20)]
    vol = _vol(keys, weight=[1.0] * 13 + [0.0])                                          # the last voxel is stored and no node: it always stays
    seq = np.asarray(keys, np.int32)[::-1].copy()
    c = CT.components(vol, 0.01)
    assert CT.removed_components(c["sizes"], min_voxels, keep_largest).tolist() == [i in gone for i in range(5)]
    out, order, counts = CT.prune_components(vol, seq, 0.01, min_voxels=min_voxels, keep_largest=keep_largest)
    leaves = {tuple(k) for k, lab in zip(c["keys"].tolist(), c["label"]) if lab in gone}
    assert counts == [14, len(leaves), 13, 5, len(gone)]
    assert [tuple(k) for k in out["keys"].tolist()] == [k for k in keys if k not in leaves] and (20, 20, 20) in [tuple(k) for k in out["keys"].tolist()]
    assert [tuple(k) for k in order.tolist()] == [tuple(k) for k in seq.tolist() if tuple(k) not in leaves]
    for k in ("sdf", "weight", "color", "first_frame"):
        assert len(out[k]) == 14 - len(leaves)
