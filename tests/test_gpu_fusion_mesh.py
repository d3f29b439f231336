"""-m gpu: i3d_fusion_extract_mesh on the device against its numpy statement (fusion_mesh_twin.py) and against the existing route to a mesh
(finish, export, Context.set_grid, Context.extract_mesh), bit for bit: positions as uint32, colours, faces and every stats field.  No tolerance anywhere.

The state of a volume is read with Fusion.debug_voxels over a dense box, as the merge tests do (test_gpu_fusion_merge.scenes).  I3D_ERR_CAPACITY needs 2^31 face
indices or vertices and is not covered."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import fusion_cases as FC
import fusion_mesh_twin as MT
from fusion_cases import fusion_frames, scenes  # noqa: F401  (fixtures)
from intrinsic3d_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.gpu

VS, VS2 = FC.VS, FC.VS2
F = np.float32
FIELDS = ("found", "sdf", "weight", "color", "first_frame")


@pytest.fixture(scope="module")
def tables():
    ntri, tri, _ = B.mc_tables()
    return ntri, tri


def _volume(f, box):
    """every stored voxel of f inside the box, as the twin's volume"""
    dv = f.debug_voxels(box); s = dv["found"]
    return dict(keys=box[s], sdf=dv["sdf"][s], weight=dv["weight"][s], color=dv["color"][s])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def _same_mesh(got, want):
    """got: (v, c, f, stats) of the device; want: the twin's dict"""
    v, c, f, st = got
    assert st == want["stats"], (st, want["stats"])
    assert v.shape == want["vertices"].shape and np.array_equal(_bits(v), _bits(want["vertices"]))
    assert np.array_equal(c, want["colors"]) and c.dtype == np.uint8
    assert f.dtype == np.int32 and np.array_equal(f, want["faces"])


def _same_state(a, b):
    for k in FIELDS:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


# ---- 1. the device against the twin on live volumes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["overlapping", "textured", "pow2"])
def test_live_volume_equals_twin(scenes, tables, name):
    s = scenes[name]
    with s.a() as A:
        vol = _volume(A, s.box)
        got = A.extract_mesh(stats=True)
        want = MT.mesh(vol, s.vs, tables)
        _same_mesh(got, want)
        st = got[3]
        assert st["faces"] > 500 and st["stored"] == int((vol["weight"] != 0).sum()) and st["vertices"] == len(got[0]) and st["faces"] == len(got[2])
        if name == "textured":
            assert len(np.unique(got[1], axis=0)) > 50                                             # colours that vary
        mw = float(np.median(vol["weight"][vol["weight"] != 0]))
        got2 = A.extract_mesh(min_weight=mw, stats=True)
        want2 = MT.mesh(vol, s.vs, tables, min_weight=mw)
        _same_mesh(got2, want2)
        assert 0 < got2[3]["valid_cells"] < st["valid_cells"]
        print(f"{name}: {st}; twins {int((want['vertex_code'] >= 4).sum())}, colour conflicts {want['direction_colour_conflicts']}; min_weight {mw}: {got2[3]['faces']} faces")


def test_all_negative_keys_equal_twin(scenes, tables):
    s = scenes["pow2"]; m = np.array((-70, -65, -80), np.int64)
    with B.Fusion(VS2, 0.1, 10.0, initial_capacity=1 << 16) as A, s.b() as Bv:
        A.merge(Bv, np.concatenate([np.zeros(3), m * VS2]))
        box = FC.dense(s.lo + m, s.hi + m)
        vol = _volume(A, box)
        assert (vol["keys"] < 0).all() and len(vol["keys"]) > 1000
        got = A.extract_mesh(stats=True)
        _same_mesh(got, MT.mesh(vol, VS2, tables))
        assert got[3]["faces"] > 500 and (got[0] < 0).all()


# ---- 2. the device against the existing route on finished volumes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["overlapping", "textured"])
def test_finished_volume_equals_the_context_route(scenes, name):
    s = scenes[name]
    with s.a() as A:
        A.finish(10)
        ex = A.export()
        v, c, f, st = A.extract_mesh(stats=True)
    with B.Context() as ctx:
        ctx.set_grid(s.vs, ex["keys"], ex["sdf"], ex["sdf"], np.zeros(len(ex["sdf"])), ex["weight"], ex["color"])
        rv, rc, rf = ctx.extract_mesh(False, 0, False)
    assert len(rf) > 500 and st["stored"] == len(ex["sdf"])
    key = lambda p: [x.tobytes() for x in (np.ascontiguousarray(p, F) + F(0))]  # noqa: E731
    mine, ref = dict(zip(key(v), map(tuple, c.tolist()))), dict(zip(key(rv), map(tuple, rc.tolist())))
    assert len(mine) == len(v) and len(ref) == len(rv) and len(v) == len(rv)                       # positions are distinct on both sides, and as many
    assert mine.keys() == ref.keys()                                                                # the same set of positions
    bad = [p for p in mine if mine[p] != ref[p]]
    assert not bad, f"{len(bad)} of {len(mine)} positions carry another colour"                    # the colour at each position
    tri = lambda vv, ff: sorted(b"".join((vv[i] + F(0)).tobytes() for i in t) for t in ff.tolist())  # noqa: E731
    assert len(f) == len(rf) and tri(v, f) == tri(rv, rf)                                           # the multiset of faces as position triples in face order
    print(f"{name}: {len(v)} vertices, {len(f)} faces, {st['degenerate_removed']} degenerate removed, on both routes")


# ---- 3. layout independence -----------------------------------------------------------------------------------------------------------------------------------------
def test_mesh_does_not_depend_on_the_table(scenes):
    s = scenes["overlapping"]
    with s.a(1 << 11) as small, s.a(1 << 16) as big:
        assert small.info()["capacity"] > 4096 and big.info()["capacity"] == 131072 != small.info()["capacity"]      # the small one started at 4 096 slots and grew
        a, b = small.extract_mesh(stats=True), big.extract_mesh(stats=True)
    assert a[3] == b[3] and a[3]["faces"] > 1000
    for x, y in zip(a[:3], b[:3]):
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


# ---- 4. hand-made content -----------------------------------------------------------------------------------------------------------------------------------------------
def _neighbourhood(vol, r):
    """per voxel of vol: its (2r+1)^3 neighbourhood is stored with weight != 0 throughout"""
    have = MT.pack(vol["keys"][vol["weight"] != 0]); have.sort()
    ok = np.ones(len(vol["keys"]), bool)
    for d in FC.dense((-r, -r, -r), (r + 1, r + 1, r + 1)).astype(np.int64):
        q = MT.pack(vol["keys"] + d); at = np.minimum(np.searchsorted(have, q), len(have) - 1)
        ok &= have[at] == q
    return ok


def _hand_made(k, w0, vs):
    """what the poke test writes into the stored voxels k [n, 3] (weights w0): (sdf, weight, color, anchor of a cell whose 8 corners are stored)"""
    rng = np.random.default_rng(11); n = len(k)
    z0 = int(np.median(k[:, 2]))
    sdf = ((k[:, 2] - z0).astype(F) * F(vs)).astype(F)                                            # an analytic field, exactly 0 on the lattice plane z = z0
    weight = np.where(w0 != 0, w0, F(1)).astype(F)
    color = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    inner = _neighbourhood(dict(keys=k, weight=weight), 1)
    lone = int(np.flatnonzero(inner & (k[:, 2] <= z0 - 4))[0]); sdf[lone] = F(0)                  # one isolated zero corner among negative neighbours
    holes = np.zeros(n, bool); holes[5::37] = True
    holes &= np.abs(k - k[lone]).max(1) > 1; weight[holes] = F(0)                                 # weight-0 holes
    nan = int(np.flatnonzero(inner & (k[:, 2] == z0) & ~holes)[3]); sdf[nan] = np.nan             # one NaN, on the plane
    below = np.flatnonzero(inner & (k[:, 2] == z0 - 1))
    return sdf, weight, color, k[below[len(below) // 2]]


def test_poked_content_equals_twin(scenes, tables):
    s = scenes["overlapping"]
    with s.a() as A:
        vol = _volume(A, s.box)
        k = vol["keys"].astype(np.int64)
        sdf, weight, color, anchor = _hand_made(k, vol["weight"], VS)
        found = A.debug_poke_voxels(k, sdf, weight, color)
        assert found.all()
        now = _volume(A, s.box)
        assert np.array_equal(now["keys"], k) and np.array_equal(_bits(now["sdf"]), _bits(sdf)) and np.array_equal(now["weight"], weight) and np.array_equal(now["color"], color)
        want = MT.mesh(now, VS, tables)
        ws = want["stats"]
        assert ws["corner_vertices"] >= 16 and ws["degenerate_removed"] >= 1 and ws["rounded_corner_occurrences"] == 0, ws      # the field delivers, before the device is looked at
        got = A.extract_mesh(stats=True)
        _same_mesh(got, want)
        assert np.isfinite(got[0]).all()
        print(f"poked: {ws}")
        # an unstored key: reported, nothing changes
        before = A.debug_voxels(s.box); info = A.info()
        far = np.array([[s.hi[0] + 50, s.hi[1] + 50, s.hi[2] + 50], k[0]], np.int32)
        assert not A.debug_voxels(far[:1])["found"][0]
        fnd = A.debug_poke_voxels(far, np.array([1.0, sdf[0]], F), np.array([3.0, weight[0]], F), np.stack([np.array([9, 9, 9], np.uint8), color[0]]))
        assert fnd.tolist() == [False, True]
        _same_state(before, A.debug_voxels(s.box)); assert A.info() == info and not A.debug_voxels(far[:1])["found"][0]
        # one cell left alone: everything poked to weight 0 except its 8 corners
        corner = ((k - anchor) >= 0).all(1) & ((k - anchor) <= 1).all(1)                           # a cell under the plane
        assert corner.sum() == 8
        w1 = np.where(corner, np.maximum(weight, F(1)), F(0)).astype(F); s1 = np.where(np.isnan(sdf), F(0), sdf)
        assert A.debug_poke_voxels(k, s1, w1, color).all()
        one = MT.mesh(_volume(A, s.box), VS, tables)
        assert one["stats"]["stored"] == 8 and one["stats"]["valid_cells"] == 1 and one["stats"]["faces"] == 2 and one["stats"]["corner_vertices"] == 4
        _same_mesh(A.extract_mesh(stats=True), one)


# ---- 5. nothing else moves -------------------------------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves(scenes, fusion_frames):
    s = scenes["overlapping"]
    _, frames, _ = fusion_frames
    h, w = s.frames[0][0].shape
    cam = dict(width=w, height=h, intr=FC.INTR, pose=frames[1][1])
    args = lambda i: (s.frames[i][0], s.frames[i][1], s.frames[i][2], s.frames[i][1], s.frames[i][3], s.frames[i][4])  # noqa: E731
    with s.a() as A, s.a() as A2, s.b() as Bv:
        v0, i0, r0, t0 = A.debug_voxels(s.box), A.info(), A.render(cam), A.track_sdf(frames[1][0], frames[1][1], FC.INTR)
        m1 = A.extract_mesh(stats=True)
        assert m1[3]["faces"] > 1000
        _same_state(v0, A.debug_voxels(s.box)); assert A.info() == i0
        FC.same_render(r0, A.render(cam))
        t1 = A.track_sdf(frames[1][0], frames[1][1], FC.INTR)
        assert np.array_equal(t0[0], t1[0]) and str(t0[1]) == str(t1[1])
        m2 = A.extract_mesh(stats=True)                                                             # and the mesh itself is reproducible
        assert m1[3] == m2[3] and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(m1[:3], m2[:3]))
        # a volume that has been meshed (and never rendered before: A2 builds no bitmap) integrates, deintegrates and merges as one that has not
        with s.a() as plain:
            A2.extract_mesh()
            for f in (A2, plain):
                assert f.integrate(*args(3)) == 2
                f.deintegrate(0, *args(0))
                assert f.merge(Bv)["ordinal"] == 3
                if f is A2:
                    f.extract_mesh()
            _same_state(A2.debug_voxels(s.box), plain.debug_voxels(s.box)); assert A2.info() == plain.info()
            FC.same_render(A2.render(cam), plain.render(cam))                                     # no stale bitmap: the extract built and dropped none
    with s.a() as A, s.a() as fresh:                                                                # a finished volume's export() is unchanged
        A.finish(10); a = A.export()
        A.extract_mesh()
        b = A.export(); c = fresh.export()
        for k in ("keys", "sdf", "weight", "color"):
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
        with pytest.raises(B.I3DError, match="i3d_fusion_integrate"):                               # and it is still finished
            A.integrate(*args(0))


# ---- 6. edges ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    nv = int([x for x in lines if x.startswith("element vertex")][0].split()[-1]); nf = int([x for x in lines if x.startswith("element face")][0].split()[-1])
    assert "format binary_little_endian 1.0" in lines and "property uchar red" in lines
    vt = np.frombuffer(body[:15 * nv], np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    ft = np.frombuffer(body[15 * nv:], np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    assert len(ft) == nf and (ft["n"] == 3).all()
    return vt["p"].copy(), vt["c"].copy(), ft["i"].copy()


def test_empty_and_surfaceless_volumes(scenes):
    s = scenes["overlapping"]
    L = B.load()
    with B.Fusion(VS, 0.1, 10.0) as E:
        assert L.i3d_fusion_get_mesh(E.h, None, None, None) == 4 and "no mesh" in L.i3d_fusion_last_error(E.h).decode()      # I3D_ERR_STATE before any extract
        v, c, f, st = E.extract_mesh(stats=True)
        assert v.shape == (0, 3) and c.shape == (0, 3) and f.shape == (0, 3) and not any(st.values())
        assert L.i3d_fusion_get_mesh(E.h, None, None, None) == 0
        with pytest.raises(B.I3DError, match="no iso-surface"):
            E.export_mesh_ply("/dev/null")
    with s.a() as A:
        vol = _volume(A, s.box); n = len(vol["keys"])
        assert A.debug_poke_voxels(vol["keys"], np.full(n, 0.01, F), np.ones(n, F), vol["color"]).all()      # no sign change anywhere
        v, c, f, st = A.extract_mesh(stats=True)
        assert len(v) == 0 and len(f) == 0 and st["stored"] == n and st["valid_cells"] > 1000
        assert not any(st[k] for k in ("surface_cells", "raw_triangles", "vertices", "corner_vertices", "faces", "degenerate_removed", "rounded_corner_occurrences"))


def test_vertices_without_faces(scenes, tables):
    """one zero corner in a negative field: 8 triangles, all degenerate and dropped, their one vertex kept - a mesh with vertices and no face"""
    s = scenes["overlapping"]
    with s.a() as A:
        vol = _volume(A, s.box); k = vol["keys"].astype(np.int64); n = len(k)
        inner = _neighbourhood(dict(keys=k, weight=np.ones(n, F)), 1)
        sdf = np.full(n, -0.5 * VS, F); sdf[np.flatnonzero(inner)[0]] = F(0)
        assert A.debug_poke_voxels(k, sdf, np.ones(n, F), vol["color"]).all()
        want = MT.mesh(_volume(A, s.box), VS, tables)
        assert want["stats"]["vertices"] == 1 and want["stats"]["faces"] == 0 and want["stats"]["degenerate_removed"] == 8
        _same_mesh(A.extract_mesh(stats=True), want)


def test_invalid_arguments_leave_the_outputs_alone(scenes):
    s = scenes["overlapping"]
    L = B.load()
    with s.a() as A:
        good = A.extract_mesh(stats=True)
        nv, nf = C.c_int64(-7), C.c_int64(-9); st = B.FusionMeshStats(); st.faces = 77

        def refused(desc, word, path=False):
            call = (lambda: L.i3d_fusion_export_mesh_ply(A.h, desc, b"/nonexistent/x.ply")) if path else \
                   (lambda: L.i3d_fusion_extract_mesh(A.h, desc, C.byref(nv), C.byref(nf), C.byref(st)))
            assert call() == 1 and word in L.i3d_fusion_last_error(A.h).decode(), L.i3d_fusion_last_error(A.h).decode()
            assert nv.value == -7 and nf.value == -9 and st.faces == 77
            v = np.zeros_like(good[0]); c = np.zeros_like(good[1]); f = np.zeros_like(good[2])
            assert L.i3d_fusion_get_mesh(A.h, B._p(v), B._p(c), B._p(f)) == 0                       # the mesh in the handle is still the last good one
            assert np.array_equal(_bits(v), _bits(good[0])) and np.array_equal(c, good[1]) and np.array_equal(f, good[2])

        assert L.i3d_fusion_extract_mesh(None, C.byref(B.fusion_mesh_desc_default()), C.byref(nv), C.byref(nf), C.byref(st)) == 1
        for path in (False, True):
            refused(None, "null descriptor", path)
            refused(C.byref(B.fusion_mesh_desc_default(min_weight=-1.0)), "min_weight", path)
            refused(C.byref(B.fusion_mesh_desc_default(min_weight=float("nan"))), "min_weight", path)
            refused(C.byref(B.fusion_mesh_desc_default(min_weight=float("inf"))), "min_weight", path)
            refused(C.byref(B.fusion_mesh_desc_default(largest_component_only=2)), "largest_component_only", path)
            refused(C.byref(B.fusion_mesh_desc_default(largest_component_only=-1)), "largest_component_only", path)
        assert L.i3d_fusion_export_mesh_ply(A.h, C.byref(B.fusion_mesh_desc_default()), None) == 1 and "null path" in L.i3d_fusion_last_error(A.h).decode()
        with pytest.raises(ValueError):
            B.fusion_mesh_desc_default(no_such_field=1)


def test_largest_component_and_ply(scenes, tables, tmp_path):
    s = scenes["overlapping"]
    with s.a() as A:
        vol = _volume(A, s.box); k = vol["keys"].astype(np.int64)
        with np.errstate(invalid="ignore"):
            outside = dict(keys=k, weight=np.where((vol["weight"] != 0) & (vol["sdf"] > 0), F(1), F(0)))
        room = _neighbourhood(outside, 1) & (vol["sdf"] > 1.5 * VS)                                 # all 26 neighbours stored, weighted and outside the surface
        assert room.any()
        sel = np.flatnonzero(room)[:1]
        assert A.debug_poke_voxels(k[sel], np.array([-0.4 * VS], F), vol["weight"][sel], vol["color"][sel]).all()      # a detached blob: one voxel inside
        v, c, f, st = A.extract_mesh(stats=True)
        _same_mesh((v, c, f, st), MT.mesh(_volume(A, s.box), VS, tables))
        lv, lc, lf, lst = A.extract_mesh(largest_component_only=True, stats=True)
        wv, wc, wf = B.mesh_remove_loose_components(v, c, f)
        at_blob = lambda p: int((np.abs(p / F(VS) - k[sel[0]]).max(1) < 1).sum())                  # noqa: E731
        assert at_blob(v) == 6 and at_blob(wv) == 0 and len(f) - len(wf) >= 8                       # the blob, an octahedron, was there and is gone
        assert np.array_equal(_bits(lv), _bits(wv)) and np.array_equal(lc, wc) and np.array_equal(lf, wf)
        assert lst["vertices"] == len(wv) and lst["faces"] == len(wf)
        assert {q: x for q, x in lst.items() if q not in ("vertices", "faces")} == {q: x for q, x in st.items() if q not in ("vertices", "faces")}
        # a PLY written from the live volume reads back to the same arrays
        A.export_mesh_ply(tmp_path / "live.ply")
        pv, pc, pf = _read_ply(tmp_path / "live.ply")
        assert np.array_equal(_bits(pv), _bits(v)) and np.array_equal(pc, c) and np.array_equal(pf, f)
        A.export_mesh_ply(tmp_path / "largest.ply", largest_component_only=True, min_weight=0.0)
        pv, pc, pf = _read_ply(tmp_path / "largest.ply")
        assert np.array_equal(_bits(pv), _bits(wv)) and np.array_equal(pc, wc) and np.array_equal(pf, wf)
        gv, gc, gf = (np.zeros_like(lv), np.zeros_like(lc), np.zeros_like(lf))
        assert B.load().i3d_fusion_get_mesh(A.h, B._p(gv), B._p(gc), B._p(gf)) == 0                  # export_mesh_ply leaves the handle's mesh as it was
        assert np.array_equal(_bits(gv), _bits(lv)) and np.array_equal(gf, lf)


# ---- 7. the app's opt-in key ----------------------------------------------------------------------------------------------------------------------------------------------
def test_app_fusion_output_mesh_live(tmp_path):
    """app_fusion with `output_mesh_live` writes the live volume's mesh before finish and leaves every other output byte for byte; the file is the mesh
    Fusion.extract_mesh gives on the same frames"""
    import subprocess
    from intrinsic3d_amd import synthetic
    import make_dataset
    sc = synthetic.make_scene(radius_vox=12, K=3, width=96, height=72, levels=1, seed=9)
    app = os.path.join(ROOT, "apps", "app_fusion")
    assert os.path.exists(app), "apps/app_fusion has not been built (run __graft_entry__.build())"
    out = {}
    for tag in ("plain", "live"):
        d = tmp_path / tag; d.mkdir()
        s_yml, _ = make_dataset.write_dataset(str(d), sc, grid_levels=1, rgbd_levels=1, iterations=1)
        if tag == "live":
            with open(d / "fusion.yml", "a") as fh:
                fh.write('output_mesh_live: "./fusion/mesh_live.ply"\n')
        r = subprocess.run([app, "-s", s_yml, "-f", str(d / "fusion.yml")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        vs = f"{float(sc['voxel_size']):g}"
        out[tag] = (open(d / "fusion" / f"mesh_{vs}.ply", "rb").read(), open(d / "fusion" / f"volume_{vs}.tsdf", "rb").read())
        assert (d / "fusion" / "mesh_live.ply").exists() == (tag == "live")
    assert out["plain"] == out["live"] and len(out["plain"][0]) > 10000
    v, c, f = _read_ply(tmp_path / "live" / "fusion" / "mesh_live.ply")
    sensor = B.Sensor(tmp_path / "live" / "rgbd", 0, 0.1, 10.0)
    with B.Fusion(sc["voxel_size"], 0.1, 10.0, np.zeros(6, np.float32), initial_capacity=1 << 21) as vol:
        for i in range(sensor.num_frames):
            vol.integrate(sensor.depth(i), sensor.depth_intrinsics, sensor.color(i), sensor.color_intrinsics, sensor.pose(i), 2)
        wv, wc, wf = vol.extract_mesh()
    assert len(f) > 500 and np.array_equal(_bits(v), _bits(wv)) and np.array_equal(c, wc) and np.array_equal(f, wf)
