"""-m gpu: i3d_fusion_components / i3d_fusion_prune_components on the device against their numpy statement (fusion_components_twin.py), bit
for bit: keys, label, sizes and counts.  Hand-made volumes go in through Fusion.insert_records: the seams of the "next entry is the +x neighbour" shortcut, deep
and late-merging shapes, a box near the percolation threshold (many components, ties), the two criteria; then fused scenes with and without a detached blob, the
relation to the mesh, that labelling changes nothing, the removal against the twin and under a later frame and a render, the errors, and app_fusion."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fusion_cases as FC
import fusion_components_twin as CT
import fusion_deintegrate_twin as DT
import fusion_load_twin as LT
import fusion_merge_twin as MT
import fusion_mesh_twin as MESH
import fusion_prune_twin as PT
from fusion_cases import fusion_frames, scenes  # noqa: F401  (fixtures)
from intrinsic3d_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

F = np.float32
VS = 0.01
FIELDS = ("sdf", "weight", "color")
STATE = ("found",) + FIELDS + ("first_frame",)
RECORD = ("keys", "sdf", "weight", "color")
OK, INVALID, ERR_STATE = 0, 1, 4


# ---- volumes by hand ------------------------------------------------------------------------------------------------------------------------------------------------
def _rec(keys, sdf=None, weight=None):
    keys = np.ascontiguousarray(np.asarray(keys, np.int32).reshape(-1, 3)); n = len(keys)
    assert len(np.unique(PT.pack(keys))) == n
    return dict(keys=keys, sdf=np.full(n, 0.002, F) if sdf is None else np.asarray(sdf, F), weight=np.ones(n, F) if weight is None else np.asarray(weight, F),
                color=(np.arange(3 * n).reshape(n, 3) % 251).astype(np.uint8))


def _loaded(rec, capacity=1 << 12, vs=VS):
    f = B.Fusion(vs, 0.1, 10.0, initial_capacity=capacity)
    if len(rec["keys"]):
        f.insert_records(**rec)
    return f


def _same(got, want, what=""):
    for k in ("nodes", "components", "largest"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ("keys", "label", "sizes"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()) if got[k].shape == want[k].shape else "shape")


def _run(x0, x1, y, z):
    return [(x, y, z) for x in range(x0, x1)]


def _serpentine(origin=(0, 0, 0), rows=16, length=31, planes=8):
    """one path: x-rows at every other y joined at alternating ends, planes at every other z joined at alternating corners; its diameter is its length"""
    k = []
    for p in range(planes):
        z = 2 * p
        for r in range(rows):
            k += _run(0, length, 2 * r, z)
            if r + 1 < rows:
                k.append((length - 1 if r % 2 == 0 else 0, 2 * r + 1, z))
        if p + 1 < planes:
            k.append((0, 2 * (rows - 1) if p % 2 == 0 else 0, z + 1))
    return np.asarray(k, np.int64) + np.asarray(origin)


def _comb(origin=(0, 0, 0), axis=0):
    """64 runs of 64 voxels joined only by a spine at their far end; along x (axis 0, runs at every other y) or along z (axis 2, runs at every other x)"""
    k = [(i, 2 * r, 0) for r in range(64) for i in range(64)] + [(64, j, 0) for j in range(127)]
    k = np.asarray(k, np.int64)
    if axis == 2:
        k = k[:, [1, 2, 0]]                                                    # (run coordinate, row, 0) -> (row, 0, run coordinate)
    return k + np.asarray(origin)


def _random_box(seed=4, side=24, density=0.30, origin=(-7, -11, 3)):
    rng = np.random.default_rng(seed)
    box = FC.dense((0, 0, 0), (side, side, side)).astype(np.int64)
    return box[rng.random(len(box)) < density] + np.asarray(origin)


SHAPES = {
    "one": [(3, -4, 5)],
    "run63": _run(0, 63, 0, 0), "run64": _run(0, 64, 0, 0), "run65": _run(0, 65, 0, 0), "run255": _run(0, 255, 0, 0), "run256": _run(0, 256, 0, 0),
    "run257": _run(0, 257, 0, 0),
    "across_zero": _run(-40, 41, 0, 0),
    "negative": _run(-300, -230, -5, -9) + _run(-280, -270, -4, -9) + [(-1000, -1000, -1000)],
    "rows_touching": _run(0, 70, 3, 0) + _run(5, 80, 4, 0),
    "rows_apart": _run(0, 70, 3, 0) + _run(5, 80, 5, 0),
    "next_in_key_order": [(9, 2, 1), (4, 3, 1)] + _run(20, 25, 3, 1) + _run(-6, -2, 4, 1),
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_smallest_shapes(name):
    rec = _rec(SHAPES[name])
    with _loaded(rec) as f:
        got = f.components()
    want = CT.components(rec, VS)
    print(f"{name}: {got['nodes']} nodes, sizes {got['sizes'].tolist()}")
    _same(got, want, name)
    if name.startswith("run") or name in ("one", "across_zero", "rows_touching"):
        assert got["components"] == 1 and got["largest"] == len(rec["keys"])
    if name == "rows_apart":
        assert got["sizes"].tolist() == [75, 70]
    if name == "next_in_key_order":
        assert got["sizes"].tolist() == [5, 4, 1, 1]


@pytest.fixture(scope="module")
def deep():
    """the serpentine, the two combs, and all three as pieces of one volume with the random box between them; each with the twin's answer"""
    parts = dict(serpentine=_serpentine(), comb_x=_comb(), comb_z=_comb(axis=2))
    parts["together"] = np.concatenate([_serpentine((-50, 40, -30)), _comb((100, -200, 7)), _comb((-300, 9, 100), axis=2), _random_box()])
    out = {}
    for name, keys in parts.items():
        rng = np.random.default_rng(len(keys))
        rec = _rec(keys[rng.permutation(len(keys))])
        out[name] = (rec, CT.components(rec, VS))
    assert out["serpentine"][1]["components"] == 1 and 3900 < out["serpentine"][1]["nodes"] < 4200
    assert out["comb_x"][1]["components"] == out["comb_z"][1]["components"] == 1 and out["comb_x"][1]["nodes"] == 64 * 64 + 127
    assert out["together"][1]["sizes"][:3].tolist() == [64 * 64 + 127, 64 * 64 + 127, out["serpentine"][1]["nodes"]]
    return out


@pytest.mark.parametrize("name", ["serpentine", "comb_x", "comb_z", "together"])
def test_depth_and_late_merges(deep, name):
    rec, want = deep[name]
    with _loaded(rec) as f:
        got = f.components()
    print(f"{name}: {got['nodes']} nodes in {got['components']} components, the largest {got['largest']}")
    _same(got, want, name)


@pytest.fixture(scope="module")
def percolating():
    keys = _random_box()
    rec = _rec(keys)
    want = CT.components(rec, VS)
    sizes = want["sizes"]
    assert want["components"] > 100 and (np.diff(sizes[sizes > 1]) == 0).any() and sizes[0] > 100, (want["components"], sizes[:10])
    return rec, want


def test_many_components_whatever_the_order_the_capacity_or_the_run(percolating):
    rec, want = percolating
    perm = np.random.default_rng(12).permutation(len(rec["keys"]))
    shuffled = {k: np.ascontiguousarray(v[perm]) for k, v in rec.items()}
    runs = []
    for r, cap in ((rec, 1 << 12), (shuffled, 1 << 12), (rec, 1 << 17)):
        with _loaded(r, capacity=cap) as f:
            runs.append(f.components()); runs.append(f.components())
            caps = f.info()["capacity"]
        print(f"initial capacity {cap}: capacity {caps}, {runs[-1]['components']} components, sizes {runs[-1]['sizes'][:8].tolist()} ...")
    for got in runs:
        _same(got, want)


def _cube(lo, side=3):
    return (FC.dense((0, 0, 0), (side, side, side)).astype(np.int64) + np.asarray(lo)).tolist()


def test_criteria_decide_what_a_node_is():
    a, b, bridge = _cube((0, 0, 0)), _cube((7, 0, 0)), _run(3, 7, 1, 1)
    keys = np.asarray(a + b + bridge)
    n = len(keys)
    light = _rec(keys, weight=[1.0] * 54 + [0.0] * 4)
    far = _rec(keys, sdf=[0.002] * 54 + [0.05, -0.05, 0.05, -0.02])
    with _loaded(light) as f:
        two, one = f.components(), f.components(min_weight=-1.0)
        half = f.components(min_weight=1.0)
    _same(two, CT.components(light, VS)); _same(one, CT.components(light, VS, min_weight=-1.0)); _same(half, CT.components(light, VS, min_weight=1.0))
    assert two["sizes"].tolist() == [27, 27] and one["sizes"].tolist() == [n] and half["nodes"] == 0 and len(half["keys"]) == 0
    with _loaded(far) as f:
        whole, cut, edge = f.components(), f.components(max_abs_sdf=0.03), f.components(max_abs_sdf=0.05)
    _same(whole, CT.components(far, VS)); _same(cut, CT.components(far, VS, max_abs_sdf=0.03)); _same(edge, CT.components(far, VS, max_abs_sdf=0.05))
    assert whole["sizes"].tolist() == [n] and cut["sizes"].tolist() == [28, 27] and edge["sizes"].tolist() == [n]      # |s| == max_abs_sdf is a node


# ---- fused scenes ---------------------------------------------------------------------------------------------------------------------------------------------------
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


def _volume(st, box):
    s = st["found"]
    return MT.volume(box[s], st["sdf"][s], st["weight"][s], st["color"][s], st["first_frame"][s])


def _by_key(vol):
    return LT.volume_of(vol["keys"], vol["sdf"], vol["weight"], vol["color"], vol["first_frame"])


def _same_records(a, b):
    assert len(a["sdf"]) == len(b["sdf"]), (len(a["sdf"]), len(b["sdf"]))
    for k in RECORD:
        assert np.array_equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))


def _masked(st, found):
    """a state over the box with everything outside `found` as debug_voxels reports a key that is not stored"""
    out = dict(found=found.copy(), sdf=np.where(found, st["sdf"], F(0)), weight=np.where(found, st["weight"], F(0)),
               color=np.where(found[:, None], st["color"], np.uint8(0)))
    if "first_frame" in st:
        out["first_frame"] = np.where(found, st["first_frame"], -1)
    return out


def _blob_place(vol, within=None):
    """the anchor a of a 2x2x2 block whose whole 4x4x4 neighbourhood a + [-1, 2]^3 is stored - with a weight and outside the surface, or, where `within` is given
    (packed keys), anywhere as long as the block lies among those keys"""
    k = np.asarray(vol["keys"], np.int64)
    pk = np.sort(PT.pack(k if within is not None else k[(vol["weight"] > 0) & (vol["sdf"] > 0)]))
    ok = np.ones(len(k), bool)
    for d in FC.dense((-1, -1, -1), (3, 3, 3)).astype(np.int64):
        ok &= np.isin(PT.pack(k + d), pk)
        if within is not None and d.min() >= 0 and d.max() <= 1:
            ok &= np.isin(PT.pack(k + d), within)
    assert ok.any()
    return k[np.flatnonzero(ok)[len(np.flatnonzero(ok)) // 2]]


def _poke_blob(f, vol, a, vs, present=True):
    """the block a + {0,1}^3 with one corner inside the surface, cut off from everything by a shell of weightless voxels; present=False: the block weightless too"""
    by = {p: i for i, p in enumerate(PT.pack(vol["keys"]).tolist())}
    hood = FC.dense((-1, -1, -1), (3, 3, 3)).astype(np.int64) + a
    block = ((hood >= a) & (hood <= a + 1)).all(1)
    at = np.array([by[p] for p in PT.pack(hood).tolist()])
    sdf = np.where(block, F(0.6) * F(vs), vol["sdf"][at]).astype(F); sdf[np.flatnonzero(block)[0]] = F(-0.4) * F(vs)
    weight = np.where(block & present, F(1), F(0)).astype(F)
    assert f.debug_poke_voxels(hood.astype(np.int32), sdf, weight, vol["color"][at]).all()
    return hood[block]


@pytest.fixture(scope="module")
def tables():
    ntri, tri, _ = B.mc_tables()
    return ntri, tri


@pytest.mark.parametrize("blob", [False, True])
@pytest.mark.parametrize("name", ["overlapping", "textured"])
def test_fused_scenes_equal_the_twin_and_faces_stay_inside_a_component(scenes, tables, name, blob):
    s = scenes[name]
    with _fuse(s, len(s.frames)) as f:
        if blob:
            vol0 = _volume(_state(f, s.box), s.box)
            block = _poke_blob(f, vol0, _blob_place(vol0), s.vs)
        vol = _volume(_state(f, s.box), s.box)
        got = f.components()
        everything = f.components(min_weight=-1.0)
        v, c, faces = f.extract_mesh()
    want = CT.components(vol, s.vs)
    print(f"{name}, blob {blob}: {len(vol['keys'])} stored, {got['nodes']} nodes in {got['components']} components, sizes {got['sizes'][:6].tolist()}; "
          f"every stored voxel: {everything['components']} components")
    _same(got, want); _same(everything, CT.components(vol, s.vs, min_weight=-1.0))
    assert got["nodes"] == int((vol["weight"] > 0).sum()) and everything["nodes"] == len(vol["keys"]) and got["largest"] > 1000
    # section 39.1 item 7: the three owner voxels of a face carry one label.  The owners are the twin's names of the vertices, which are the device's bit for bit
    m = MESH.mesh(vol, s.vs, tables)
    assert np.array_equal(v.view(np.uint32), m["vertices"].view(np.uint32)) and np.array_equal(faces, m["faces"]) and len(faces) > 1000
    pk = PT.pack(got["keys"]); owner = PT.pack(m["vertex_owner"])
    at = np.searchsorted(pk, owner)
    assert np.array_equal(pk[np.minimum(at, len(pk) - 1)], owner)                          # every owner is a node
    lab = got["label"][at][faces]
    assert np.all(lab[:, 0] == lab[:, 1]) and np.all(lab[:, 0] == lab[:, 2])
    if blob:
        mine = got["label"][np.searchsorted(pk, PT.pack(block))]
        assert len(set(mine.tolist())) == 1 and mine[0] > 0 and got["sizes"][mine[0]] == 8          # a component of its own
        assert (lab[:, 0] == mine[0]).sum() >= 1                                                    # with its piece of the mesh


def _camera(s, i):
    d, intr, _, T, _ = s.frames[i]
    return dict(width=d.shape[1], height=d.shape[0], intr=np.asarray(intr, np.float64), pose=B.pose_mat_to_vec6(T))


def _readers(f, s):
    cam = _camera(s, 1)
    start = _camera(s, 2)["pose"] + np.array([0.004, -0.003, 0.002, 0.003, -0.002, 0.004])
    return dict(state=_state(f, s.box), info=f.info(), order=f.debug_insertion_order(), render=f.render(cam), track=f.track_sdf(s.frames[2][0], start, cam["intr"]))


def _same_readers(a, b):
    _same_state(a["state"], b["state"])
    assert a["info"] == b["info"] and np.array_equal(a["order"], b["order"])
    FC.same_render(a["render"], b["render"])
    assert np.array_equal(a["track"][0], b["track"][0]) and a["track"][1] == b["track"][1]


def test_labelling_changes_nothing(scenes):
    s = scenes["overlapping"]
    L = B.load(); p = B._p
    with _fuse(s, 3) as f, _fuse(s, 3) as plain:
        k = np.zeros((4, 3), np.int32)
        assert L.i3d_fusion_get_components(f.h, p(k), None, None) == ERR_STATE and "labelled" in L.i3d_fusion_last_error(f.h).decode() and not k.any()
        before = _readers(f, s)
        first = f.components()
        _same_readers(before, _readers(f, s))
        _same(f.components(max_abs_sdf=float(F(2) * F(s.vs))), CT.components(_volume(before["state"], s.box), s.vs, max_abs_sdf=float(F(2) * F(s.vs))))
        _same_readers(before, _readers(f, s))
        # the volume goes on exactly as one that was never labelled, and a finished one can be labelled
        assert f.integrate(*_args(s.frames[3 % len(s.frames)])) == plain.integrate(*_args(s.frames[3 % len(s.frames)]))
        assert f.finish(10) == plain.finish(10)
        rec = f.export()
        _same_records(rec, plain.export())
        done = f.components()
        _same(done, CT.components(_volume(_state(f, s.box), s.box), s.vs))
        _same_records(f.export(), rec)
        assert first["nodes"] > 1000 and done["nodes"] > 1000
        # the stored labelling is the last one
        keys = np.zeros((done["nodes"], 3), np.int32); label = np.zeros(done["nodes"], np.int32); sizes = np.zeros(done["components"], np.int64)
        assert L.i3d_fusion_get_components(f.h, p(keys), None, None) == OK and L.i3d_fusion_get_components(f.h, None, p(label), p(sizes)) == OK
        assert np.array_equal(keys, done["keys"]) and np.array_equal(label, done["label"]) and np.array_equal(sizes, done["sizes"])
    with B.Fusion(VS, 0.1, 10.0) as f:
        got = f.components()
        assert (got["nodes"], got["components"], got["largest"]) == (0, 0, 0) and got["keys"].shape == (0, 3) and len(got["label"]) == len(got["sizes"]) == 0
        assert f.prune_components(min_voxels=5) == dict(stored=0, removed=0, nodes=0, components=0, components_removed=0)


# ---- the removal ----------------------------------------------------------------------------------------------------------------------------------------------------
def _counts(c):
    return [c[k] for k in CT.COUNTS]


def _check_prune(f, box, vs, params, shrink):
    """one prune_components against the twin: counts, state, insertion order, capacity, and the snapshot's records"""
    st0 = _state(f, box); order0 = f.debug_insertion_order(); info0 = f.info()
    assert len(order0) == int(st0["found"].sum())
    labelled = f.components()
    counts = f.prune_components(shrink=shrink, **params)
    st1 = _state(f, box); order1 = f.debug_insertion_order(); info1 = f.info()
    n = f.snapshot(); snap = f.export()
    want, want_order, want_counts = CT.prune_components(_volume(st0, box), order0, vs, **params)
    assert _counts(counts) == want_counts, (counts, want_counts)
    got = _volume(st1, box)
    for k in ("keys",) + FIELDS + ("first_frame",):
        assert np.array_equal(got[k], want[k]), (k, len(got[k]), len(want[k]))
    assert np.array_equal(order1, want_order)
    assert info1["capacity"] == PT.capacity_after(info0["capacity"], counts["stored"] - counts["removed"], counts["removed"], shrink)
    assert {k: v for k, v in info1.items() if k not in ("capacity", "allocated")} == {k: v for k, v in info0.items() if k not in ("capacity", "allocated")}
    rec = LT.snapshot_records(_by_key(want), want_order)
    assert n == len(rec["sdf"])
    _same_records(snap, rec)
    # the handle's stored labelling is the one of before
    L = B.load(); keys = np.zeros((labelled["nodes"], 3), np.int32)
    assert L.i3d_fusion_get_components(f.h, B._p(keys), None, None) == OK and np.array_equal(keys, labelled["keys"])
    return counts, info0, info1


@pytest.mark.parametrize("shrink", [False, True])
@pytest.mark.parametrize("params", [dict(min_voxels=4), dict(keep_largest=3), dict(min_voxels=20, keep_largest=40), dict(min_voxels=2, min_weight=-1.0),
                                    dict(keep_largest=1, max_abs_sdf=0.0021)], ids=["min_voxels", "keep_largest", "both", "weight_off", "sdf"])
def test_prune_components_on_the_box_equals_the_twin(percolating, params, shrink):
    rec, _ = percolating
    rng = np.random.default_rng(2)
    rec = dict(rec, weight=np.where(rng.random(len(rec["sdf"])) < 0.1, F(0), F(1)), sdf=np.where(rng.random(len(rec["sdf"])) < 0.1, F(0.003), F(0.002)))
    lo, hi = rec["keys"].min(0) - 1, rec["keys"].max(0) + 2
    with _loaded(rec, capacity=1 << 15) as f:
        counts, info0, info1 = _check_prune(f, FC.dense(lo, hi), VS, params, shrink)
    print(f"{params}, shrink {shrink}: {counts}, capacity {info0['capacity']} -> {info1['capacity']}")
    assert 0 < counts["removed"] < counts["nodes"] <= counts["stored"] and 0 < counts["components_removed"] < counts["components"]
    assert (info1["capacity"] < info0["capacity"]) == shrink


@pytest.mark.parametrize("name", ["overlapping", "textured"])
def test_prune_components_on_a_scene_removes_the_blob(scenes, name):
    s = scenes[name]
    cam = _camera(s, 1)
    with _fuse(s, 3) as f, _fuse(s, 3) as never:
        vol0 = _volume(_state(f, s.box), s.box)
        a = _blob_place(vol0)
        block = _poke_blob(f, vol0, a, s.vs); _poke_blob(never, vol0, a, s.vs, present=False)
        with_blob = f.render(cam)
        sizes = f.components()["sizes"]
        counts, info0, info1 = _check_prune(f, s.box, s.vs, dict(min_voxels=9), True)
        st = _state(f, s.box)
        after = f.render(cam); without = never.render(cam)
    print(f"{name}: sizes {sizes[:6].tolist()}, {counts}, capacity {info0['capacity']} -> {info1['capacity']}; the render differs from the one with the blob in "
          f"{int((with_blob['depth'] != after['depth']).sum())} pixels")
    assert counts["removed"] >= 8 and counts["components_removed"] >= 1 and counts["components"] - counts["components_removed"] >= 1
    assert not st["found"][np.isin(PT.pack(s.box), PT.pack(block))].any()
    FC.same_render(after, without)                                             # nothing of the blob is hit: the volume that never had it renders the same
    assert after["stats"]["hits"] > 100


def test_removing_nothing_leaves_the_table_alone(scenes):
    s = scenes["textured"]
    with _fuse(s, 2) as f, _fuse(s, 2) as plain:
        before = _readers(f, s)
        c = f.components()
        for params in (dict(), dict(min_voxels=1), dict(keep_largest=c["components"]), dict(min_voxels=int(c["sizes"][-1]), keep_largest=c["components"] + 5)):
            counts = f.prune_components(shrink=True, **params)
            assert _counts(counts) == [len(before["order"]), 0, c["nodes"], c["components"], 0], (params, counts)
        assert PT.capacity_after(before["info"]["capacity"], len(before["order"]), 1, True) < before["info"]["capacity"]      # a shrink that acted would show
        _same_readers(before, _readers(f, s))
        assert f.integrate(*_args(s.frames[2])) == plain.integrate(*_args(s.frames[2])) == 2
        _same_state(_state(f, s.box), _state(plain, s.box))
        assert np.array_equal(f.debug_insertion_order(), plain.debug_insertion_order())


@pytest.mark.parametrize("name", ["textured", "overlapping"])
def test_a_later_frame_reinserts_around_the_survivors(scenes, name):
    """section 38.4 case 4 on this verdict: a blob where the next frame allocates leaves with every other small component, and the frame puts its voxels back"""
    s = scenes[name]
    with _fuse(s, 2) as f, _fuse(s, 1, first=2) as fresh:
        fr = _state(fresh, s.box); order_fresh = fresh.debug_insertion_order()
        vol0 = _volume(_state(f, s.box), s.box)
        _poke_blob(f, vol0, _blob_place(vol0, within=PT.pack(s.box[fr["found"]])), s.vs)
        st0 = _state(f, s.box); order0 = f.debug_insertion_order()
        params = dict(keep_largest=1)
        counts = f.prune_components(**params)
        smp = f.debug_frame_samples(s.box, *_args(s.frames[2]))
        assert f.integrate(*_args(s.frames[2])) == 2
        st2 = _state(f, s.box); order2 = f.debug_insertion_order()
    want, want_order, want_counts = CT.prune_components(_volume(st0, s.box), order0, s.vs, **params)
    assert _counts(counts) == want_counts and 8 <= counts["removed"] < counts["nodes"]
    kept = np.isin(PT.pack(s.box), PT.pack(want["keys"]))
    pruned = _masked(st0, kept)
    gone = st0["found"] & ~kept
    assert np.array_equal(st2["found"], kept | fr["found"])
    back = gone & fr["found"]
    print(f"{name}: {counts}; {int(back.sum())} of the removed voxels inserted again by the next frame, {int((gone & ~fr['found']).sum())} stay away")
    assert back.sum() >= 8
    _same_state(st2, _masked(DT.integrate(pruned, smp, sel=st2["found"]), st2["found"]), FIELDS)
    new = order_fresh[~np.isin(LT.pack(order_fresh), LT.pack(want_order))]
    assert np.array_equal(order2, np.concatenate([want_order, new]))
    is_new = st2["found"] & ~kept
    assert np.all(st2["first_frame"][is_new] == 2) and np.array_equal(st2["first_frame"][kept], st0["first_frame"][kept])
    assert np.all(st2["first_frame"][back] == 2)


def test_refusals_leave_state_and_outputs_alone(scenes):
    s = scenes["textured"]
    L = B.load(); p = B._p
    nan, inf = float("nan"), float("inf")
    with _fuse(s, 2) as f:
        labelled = f.components()
        st0 = _state(f, s.box); order0 = f.debug_insertion_order(); info0 = f.info()
        c3 = np.full(3, -7, np.int64); c5 = np.full(5, -7, np.int64)
        assert L.i3d_fusion_components(None, 0.0, 0.0, p(c3)) == INVALID and L.i3d_fusion_get_components(None, None, None, None) == INVALID
        assert L.i3d_fusion_prune_components(None, 0.0, 0.0, 0, 0, 0, p(c5)) == INVALID
        for mw, ms in ((nan, 0.0), (inf, 0.0), (0.0, nan), (0.0, -inf)):
            assert L.i3d_fusion_components(f.h, mw, ms, p(c3)) == INVALID and "finite" in L.i3d_fusion_last_error(f.h).decode()
            assert L.i3d_fusion_prune_components(f.h, mw, ms, 1, 1, 1, p(c5)) == INVALID and "finite" in L.i3d_fusion_last_error(f.h).decode()
        assert L.i3d_fusion_components(f.h, 0.0, 0.0, None) == INVALID and "null" in L.i3d_fusion_last_error(f.h).decode()
        for mv, kl in ((-1, 0), (0, -1), (-5, -5)):
            assert L.i3d_fusion_prune_components(f.h, 0.0, 0.0, mv, kl, 1, p(c5)) == INVALID and ">= 0" in L.i3d_fusion_last_error(f.h).decode()
        assert np.all(c3 == -7) and np.all(c5 == -7)
        _same_state(_state(f, s.box), st0)
        assert np.array_equal(f.debug_insertion_order(), order0) and f.info() == info0
        again = f.components()
        _same(again, labelled)                                                  # the refused calls did not touch the stored labelling either
        assert L.i3d_fusion_prune_components(f.h, 0.0, 0.0, 0, 0, 0, None) == OK           # null counts are fine
        f.finish(0)
        rec = f.export()
        assert L.i3d_fusion_prune_components(f.h, 0.0, 0.0, 10 ** 9, 0, 1, p(c5)) == ERR_STATE and "finished" in L.i3d_fusion_last_error(f.h).decode()
        assert np.all(c5 == -7)
        _same_state(_state(f, s.box), st0)
        _same_records(f.export(), rec)
        with pytest.raises(B.I3DError):
            f.prune_components(min_voxels=10)


# ---- app_fusion: components_min_voxels --------------------------------------------------------------------------------------------------------------------------------
def test_app_fusion_components_min_voxels(fusion_frames, tmp_path):
    """the three-frame dataset of the other app_fusion tests; the app's file against the file the binding writes for the same call"""
    import make_dataset
    app = os.path.join(ROOT, "apps", "app_fusion")
    assert os.path.exists(app), "apps/app_fusion has not been built (run __graft_entry__.build())"
    _, frames, _ = fusion_frames
    sc = dict(voxel_size=FC.VS, intr=FC.INTR, keys=np.zeros((1, 3), np.int32), sdf=np.zeros(1, np.float32), weight=np.ones(1, np.float32), color=np.zeros((1, 3), np.uint8),
              frames=[dict(depth=[d], bgr=[FC.BGR]) for d, _ in frames[:3]], poses=[p for _, p in frames[:3]])
    out = tmp_path / "ds"
    yml, _ = make_dataset.write_dataset(str(out), sc)
    base = (out / "fusion.yml").read_text()
    vs = float(F(float(f"{float(FC.VS):g}")))
    sensor = B.Sensor(out / "rgbd", 0, 0.1, 10.0)                          # sensor.yml's dataset and depth range
    lo, hi = sensor.depth_range

    def through_the_binding(name, n):
        with B.Fusion(vs, lo, hi, clip=np.zeros(6, F)) as f:
            for i in range(3):
                f.integrate(sensor.depth(i), sensor.depth_intrinsics, sensor.color(i), sensor.color_intrinsics, sensor.pose(i), 2)
            sizes = f.components()["sizes"]
            counts = f.prune_components(min_voxels=n, shrink=True) if n else None
            f.finish(0)
            f.save(tmp_path / f"{name}.tsdf")
        return sizes, counts
    sizes, _ = through_the_binding("plain", 0)
    most = int(sizes[0])                                                    # every component smaller than the largest leaves
    runs = dict(plain=0, off=0, small=50, most=most)
    removed = {name: through_the_binding(name, n)[1] for name, n in runs.items()}
    sensor.close()
    print(f"component sizes {sizes[:8].tolist()}; through the binding: {removed}")
    for name, n in runs.items():
        extra = f'correct_iterations: "0"\noutput_sdf: "./fusion/{name}.tsdf"\n' + ("" if name == "plain" else f'components_min_voxels: "{n}"\n')
        (out / f"{name}.yml").write_text(base + extra)
        r = subprocess.run([app, "-s", yml, "-f", str(out / f"{name}.yml")], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.count("components:") == (1 if n else 0), r.stdout
        assert (out / "fusion" / f"{name}.tsdf").read_bytes() == (tmp_path / f"{name}.tsdf").read_bytes(), name
    assert (out / "fusion" / "off.tsdf").read_bytes() == (out / "fusion" / "plain.tsdf").read_bytes()
    (out / "negative.yml").write_text(base + 'components_min_voxels: "-3"\n')
    r = subprocess.run([app, "-s", yml, "-f", str(out / "negative.yml")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "components_min_voxels" in r.stderr
    assert removed["most"]["components_removed"] == removed["most"]["components"] - int((sizes == most).sum())
