"""No device: the surface of i3d_fusion_insert_records / _load / _snapshot / _debug_insertion_order in the header, the ABI table and the
binding, and the self-checks of their numpy statement (fusion_load_twin.py)."""
import os
import re

import numpy as np

import fusion_load_twin as LT
from intrinsic3d_amd import abi, binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("i3d_fusion_insert_records", "i3d_fusion_load", "i3d_fusion_snapshot", "i3d_fusion_debug_insertion_order")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "intrinsic3d_hip.h")).read(), flags=re.S)


def test_the_four_symbols_are_declared_bound_and_exported():
    declared = set(re.findall(r"\b(i3d_[a-z0-9_]+)\s*\(", _header()))
    table = [name for name, _, _ in abi.PROTOTYPES]
    lib = B.load()
    for name in NEW:
        assert name in declared, name
        assert table.count(name) == 1 and name in B.EXPORTS, name
        assert hasattr(lib, name), name
    # in the header's order: the three beside i3d_fusion_save, the debug entry last of the fusion debug entries
    assert table.index("i3d_fusion_save") + 1 == table.index(NEW[0]) == table.index(NEW[1]) - 1 == table.index(NEW[2]) - 2
    for method in ("insert_records", "load", "snapshot", "debug_insertion_order"):
        assert callable(getattr(B.Fusion, method)), method


def test_no_new_struct():
    """scalars and arrays only: the header's structs are still the 25 that abi.py mirrors (and i3d_lm_record, a numpy record)"""
    import ctypes
    declared = set(re.findall(r"\}\s*(i3d_[a-z0-9_]+)\s*;", _header())) - {"i3d_status", "i3d_lm_record"}
    mirrors = {v._c_name_ for v in vars(abi).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and "_c_name_" in vars(v)}
    assert len(declared) == 25 and declared == mirrors, sorted(declared ^ mirrors)


def _keys(n, seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(-40, 40, (4 * n, 3)).astype(np.int32)
    _, first = np.unique(LT.pack(k), return_index=True)
    return np.ascontiguousarray(k[np.sort(first)][:n])


def test_order_agrees_with_the_replay_and_the_closed_form():
    for n in (1, 2, 13, 200, 5000):
        k = _keys(n, n)
        assert len(k) == n
        want = LT.order(k)
        assert sorted(LT.pack(want).tolist()) == sorted(LT.pack(k).tolist())
        for mode in (0, 3):
            assert np.array_equal(LT.order(k, mode=mode), want), (n, mode)
    assert LT.order(np.zeros((0, 3), np.int32)).shape == (0, 3)


def test_reordering_on_load_is_not_idempotent():
    """Limit 2 of section 36: a saved volume is in map order, and loading it inserts in THAT order, which iterates differently again.  The order after a load is
    therefore not the order of the run that wrote the file - by the reference's own behaviour, not by a defect to be repaired here."""
    k = _keys(200, 7)
    once = LT.order(k); twice = LT.order(once)
    assert sorted(LT.pack(once).tolist()) == sorted(LT.pack(twice).tolist())
    assert not np.array_equal(once, twice)


def test_twin_snapshot_keeps_positive_weights_in_map_order():
    k = _keys(64, 3)
    rng = np.random.default_rng(3)
    rec = dict(keys=k, sdf=rng.normal(size=64).astype(np.float32), weight=rng.integers(0, 3, 64).astype(np.float32), color=rng.integers(0, 256, (64, 3)).astype(np.uint8))
    vol = LT.loaded(rec)
    assert len(vol) == 64 and all(v[3] == 0 for v in vol.values())
    snap = LT.snapshot_records(vol, k)
    on = rec["weight"] > 0
    assert len(snap["sdf"]) == int(on.sum()) and np.all(snap["weight"] > 0)
    want = LT.order(k); want = want[np.isin(LT.pack(want), LT.pack(k[on]))]
    assert np.array_equal(snap["keys"], want)
    by_key = {p: i for i, p in enumerate(LT.pack(k).tolist())}
    idx = np.array([by_key[p] for p in LT.pack(snap["keys"]).tolist()])
    assert np.array_equal(snap["sdf"], rec["sdf"][idx]) and np.array_equal(snap["weight"], rec["weight"][idx]) and np.array_equal(snap["color"], rec["color"][idx])
