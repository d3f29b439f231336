"""The numpy statement of i3d_fusion_extract_mesh (fusion_mesh_twin.py) on hand-made volumes: no GPU.

mesh() itself asserts on every volume it meshes that its weld by (owner, code) is the weld by position; every test here therefore checks that as well.

The interpolation of the reference is not symmetric in the last bit and neighbouring cells walk the x and y edges in opposite directions (edges 0, 1, 4, 5 downwards),
so the reference's weld by position leaves TWO vertices, one ulp apart, on a few percent of those edges, and a mesh welded that way is closed only up to these pairs.
The closedness of the sphere is therefore checked with every such pair taken as one vertex (vertex_code 4, 5 read as 1, 2 of the same owner) - what a weld by cell
edge would give - and the number of pairs is printed."""

import numpy as np

import fusion_mesh_twin as MT
from intrinsic3d_amd import binding as B

VS = 0.004
F = np.float32


def tables():
    ntri, tri, _ = B.mc_tables()
    return ntri, tri


def box(lo, hi):
    return np.stack(np.meshgrid(*[np.arange(lo, hi, dtype=np.int64)] * 3, indexing="ij"), -1).reshape(-1, 3)


def sphere(radius=6.0, band=3.0, centre=(0.3, -0.2, 0.1)):
    k = box(-11, 12)
    d = np.linalg.norm(k - np.asarray(centre), axis=1) - radius
    k = k[np.abs(d) <= band]; d = d[np.abs(d) <= band]
    rng = np.random.default_rng(3)
    return dict(keys=k, sdf=(d * VS).astype(F), weight=rng.integers(1, 6, len(k)).astype(F), color=rng.integers(0, 256, (len(k), 3)).astype(np.uint8))


def same_mesh(a, b):
    for key in ("vertices", "colors", "faces"):
        x, y = a[key], b[key]
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y), key
    assert a["stats"] == b["stats"]


def edge_ids(m):
    """vertex ids with the two directions of a cell edge taken as one vertex"""
    code = np.where(m["vertex_code"] >= 4, m["vertex_code"] - 3, m["vertex_code"])
    _, ids = np.unique(np.concatenate([m["vertex_owner"], code[:, None]], 1), axis=0, return_inverse=True)
    return ids.reshape(-1)


def test_sphere_is_closed_and_welded_by_position():
    v = sphere(); m = MT.mesh(v, VS, tables())
    assert (v["keys"] < 0).any(0).all() and (v["keys"] > 0).any(0).all()
    s = m["stats"]
    assert s["faces"] > 500 and s["degenerate_removed"] == 0 and s["corner_vertices"] == 0 and s["faces"] == s["raw_triangles"]
    # the vertex count is the number of distinct positions
    assert len(np.unique((m["vertices"] + F(0)).view(np.uint32), axis=0)) == len(m["vertices"]) == s["vertices"]
    # no degenerate face survives
    f = m["faces"]
    assert not MT.degenerate(m["vertices"][f[:, 0]], m["vertices"][f[:, 1]], m["vertices"][f[:, 2]]).any()
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 0] != f[:, 2]).all() and (f[:, 1] != f[:, 2]).all()
    # closed, genus 0 - up to the reference's last-bit vertex pairs (module docstring)
    ids = edge_ids(m); g = ids[f]
    e = np.sort(np.concatenate([g[:, [0, 1]], g[:, [1, 2]], g[:, [2, 0]]]), 1)
    ue, cnt = np.unique(e, axis=0, return_counts=True)
    assert (cnt == 2).all()
    V = len(np.unique(ids))
    assert V - len(ue) + len(f) == 2
    pairs = len(m["vertices"]) - V
    print(f"sphere: {s['vertices']} vertices, {s['faces']} faces, {pairs} edges carry two vertices one ulp apart, {m['direction_colour_conflicts']} colour conflicts")
    assert pairs == int((m["vertex_code"] >= 4).sum())


def test_input_order_does_not_matter():
    v = sphere(); m = MT.mesh(v, VS, tables())
    p = np.random.default_rng(1).permutation(len(v["keys"]))
    same_mesh(m, MT.mesh({k: a[p] for k, a in v.items()}, VS, tables()))


def _touching(v, bad):
    """valid cells (anchors) of v that have one of the voxels `bad` (bool per voxel) as a corner"""
    have = {tuple(k): i for i, k in enumerate(v["keys"].tolist())}
    n = 0
    for k in v["keys"].tolist():
        c = [have.get((k[0] + d[0], k[1] + d[1], k[2] + d[2])) for d in MT.CORNER.tolist()]
        if all(i is not None and v["weight"][i] != 0 and np.isfinite(v["sdf"][i]) for i in c) and any(bad[i] for i in c):
            n += 1
    return n


def test_min_weight_removes_exactly_the_cells_that_touch():
    v = sphere(); full = MT.mesh(v, VS, tables())
    low = v["weight"] < 2
    assert 50 < low.sum() < len(low) - 50
    m = MT.mesh(v, VS, tables(), min_weight=2.0)
    assert m["stats"]["valid_cells"] == full["stats"]["valid_cells"] - _touching(v, low) < full["stats"]["valid_cells"]
    gone = dict(v, weight=np.where(low, F(0), v["weight"]))                      # the same cells go when these voxels are not there at all
    want = MT.mesh(gone, VS, tables())
    want["stats"]["stored"] = m["stats"]["stored"]
    for key in ("vertices", "colors", "faces"):
        assert np.array_equal(m[key], want[key]), key
    assert m["stats"] == want["stats"] and 0 < m["stats"]["faces"] < full["stats"]["faces"]


def test_exact_zeros_on_a_lattice_plane_give_corner_vertices():
    k = box(-4, 5)
    v = dict(keys=k, sdf=(k[:, 2].astype(F) * F(VS)), weight=np.ones(len(k), F), color=np.random.default_rng(2).integers(0, 256, (len(k), 3)).astype(np.uint8))
    m = MT.mesh(v, VS, tables()); s = m["stats"]
    assert s["corner_vertices"] == s["vertices"] == 81 and (m["vertex_code"] == 0).all() and s["rounded_corner_occurrences"] == 0
    assert (m["vertices"][:, 2] == 0).all() and np.array_equal(m["vertices"], m["vertex_owner"].astype(F) * F(VS))
    assert s["faces"] == 2 * 64 and s["degenerate_removed"] == 0
    have = {tuple(q): c for q, c in zip(k.tolist(), v["color"])}
    assert np.array_equal(m["colors"], np.array([have[tuple(q)] for q in m["vertex_owner"].tolist()], np.uint8))


def test_a_single_zero_corner_gives_degenerate_triangles_whose_vertex_stays():
    k = box(-2, 3)
    sdf = np.full(len(k), F(-0.5 * VS)); sdf[(k == 0).all(1)] = F(0)
    m = MT.mesh(dict(keys=k, sdf=sdf, weight=np.ones(len(k), F), color=np.zeros((len(k), 3), np.uint8)), VS, tables()); s = m["stats"]
    assert s["raw_triangles"] == s["degenerate_removed"] == 8 and s["faces"] == 0 and len(m["faces"]) == 0
    assert s["vertices"] == s["corner_vertices"] == 1 and np.array_equal(m["vertices"], np.zeros((1, 3), F))


def test_a_nan_corner_silences_its_eight_cells_and_nothing_else():
    v = sphere(); full = MT.mesh(v, VS, tables())
    i = int(np.argmin(np.abs(v["sdf"])))
    bad = np.zeros(len(v["sdf"]), bool); bad[i] = True
    touched = _touching(v, bad)
    assert touched == 8
    nan = dict(v, sdf=v["sdf"].copy()); nan["sdf"][i] = np.nan
    m = MT.mesh(nan, VS, tables())
    assert np.isfinite(m["vertices"]).all() and m["stats"]["valid_cells"] == full["stats"]["valid_cells"] - 8
    want = MT.mesh(dict(v, weight=np.where(bad, F(0), v["weight"])), VS, tables())
    want["stats"]["stored"] = m["stats"]["stored"]
    for key in ("vertices", "colors", "faces"):
        assert np.array_equal(m[key], want[key]), key
    assert m["stats"] == want["stats"] and m["stats"]["faces"] < full["stats"]["faces"]


def test_the_soup_welded_by_position_is_the_mesh():
    v = sphere(); m = MT.mesh(v, VS, tables())
    V, C, Fc = MT.weld_by_position(m["soup_positions"], m["soup_colors"])
    assert len(V) == len(m["vertices"]) and len(Fc) == len(m["faces"])
    key = lambda p: [x.tobytes() for x in (np.asarray(p, F) + F(0))]
    mine = dict(zip(key(m["vertices"]), map(tuple, m["colors"].tolist()))); ref = dict(zip(key(V), map(tuple, C.tolist())))
    assert mine.keys() == ref.keys()
    # the colour at each position: the reference takes the first appearance's, the definition the vertex's own direction; they differ only where the two directions
    # of an edge truncate to different bytes
    assert sum(mine[p] != ref[p] for p in mine) <= m["direction_colour_conflicts"]
    tri = lambda vv, ff: sorted(b"".join((vv[i] + F(0)).tobytes() for i in f) for f in ff.tolist())
    assert tri(m["vertices"], m["faces"]) == tri(V, Fc)
    # soup order is face order: cells in ascending key, a cell's triangles in table order
    assert np.array_equal(m["vertices"][m["faces"]].view(np.uint32), (m["soup_positions"] + F(0)).view(np.uint32))


def test_empty_and_surfaceless_volumes():
    e = MT.mesh(dict(keys=np.zeros((0, 3), np.int64), sdf=np.zeros(0, F), weight=np.zeros(0, F), color=np.zeros((0, 3), np.uint8)), VS, tables())
    assert not any(e["stats"].values()) and e["vertices"].shape == (0, 3) and e["faces"].shape == (0, 3)
    k = box(0, 4)
    m = MT.mesh(dict(keys=k, sdf=np.full(len(k), F(0.01)), weight=np.ones(len(k), F), color=np.zeros((len(k), 3), np.uint8)), VS, tables())
    assert m["stats"]["valid_cells"] == 27 and m["stats"]["stored"] == 64 and m["stats"]["surface_cells"] == 0 and len(m["vertices"]) == 0
