"""i3d_cast_rays / i3d_fusion_cast_rays on the device: bit for bit against the renderer on a camera's rays, against the numpy statement
(cast_rays_twin.py) on general rays, the coherent order against the given order, invalid rays, segments, what a call must leave alone, and the fault table."""
import ctypes as C

import numpy as np
import pytest

import cast_rays_cases as cases
import cast_rays_twin as twin
import render_twin
from helpers import c2w
from intrinsic3d_amd import binding, synthetic

pytestmark = pytest.mark.gpu

ALL = binding.CAST_OUTPUTS
FUSION_ALL = ("t", "position", "normal", "status")
PLANES = ("depth", "normal", "albedo", "shading", "intensity")


def _context(sc):
    sdf_r, alb = cases.perturbed(sc)
    ctx = binding.Context(0)
    ctx.set_grid(sc["voxel_size"], sc["keys"], sc["sdf"], sdf_r, alb, sc["weight"], sc["color"])
    ctx.set_voxel_sh(np.tile(synthetic.SH_TRUE, (ctx.N, 1)))
    return ctx


def _fusion(sc):
    """the scene fused from its three keyframes and the front camera's view"""
    f = binding.Fusion(float(sc["voxel_size"]), 0.01, 10.0, initial_capacity=1 << 16)
    intr = sc["intr"].astype(np.float32)
    for k in range(sc["K"]):
        fr = sc["frames"][k]
        f.integrate(fr["depth"][0], intr, fr["bgr"][0], intr, c2w(sc["poses"][k]), 2)
    cam = cases.front_camera(sc)[0]
    _, depth, bgr = synthetic.render_frame(sc["scene"], cam["pose"], cam["intr"], cam["width"], cam["height"])
    ci = cam["intr"].astype(np.float32)
    f.integrate(depth, ci, bgr, ci, c2w(cam["pose"]), 2)
    return f


def _twin_grid(ctx):
    a = ctx.export_grid()
    _, vs, _ = ctx.grid_info()
    return render_twin.Grid(a["keys"], a["sdf_refined"], a["weight"], vs, albedo=a["albedo"], sh=ctx.get_voxel_sh())


@pytest.fixture(scope="module")
def plain():
    """the scene, its context, the twin's grid, the union of the camera's and the general rays and the twin's answer on it: computed once, changed by no test"""
    sc = cases.scene()
    ctx = _context(sc)
    grid = _twin_grid(ctx)
    cam, co, cd = cases.front_camera(sc)
    go, gd, glo, ghi = cases.general_rays(sc, grid)
    o = np.concatenate([co, go]); d = np.concatenate([cd, gd])
    lo = np.concatenate([np.zeros(len(co)), glo]); hi = np.concatenate([np.zeros(len(co)), ghi])
    general = np.arange(len(co), len(o))
    yield dict(sc=sc, ctx=ctx, grid=grid, cam=cam, n_cam=len(co), o=o, d=d, lo=lo, hi=hi, general=general, tw=twin.cast(grid, go, gd, glo, ghi))
    ctx.close()


def _same(a, b, names):
    for k in names:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["stats"] == b["stats"]


# ---- 1. equals the renderer, bit for bit -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [None, cases.SHIFT], ids=["origin", "negative_octant"])
def test_camera_rays_equal_the_renderer(shift):
    sc = cases.scene(shift=shift)
    cam, o, d = cases.front_camera(sc)
    with _context(sc) as ctx:
        for refined in (True, False):
            view = ctx.render_view(frame=-1, refined=refined, planes=PLANES, camera=cam)
            out = ctx.cast_rays(o, d, outputs=ALL, refined=refined)
            hit = view["depth"].ravel() > 0
            assert hit.sum() > 500
            assert np.array_equal(out["t"].astype(np.float32), view["depth"].ravel())
            assert np.array_equal(out["normal"], view["normal"].reshape(-1, 3))
            for k in ("albedo", "shading", "intensity"):
                assert np.array_equal(out[k], view[k].ravel()), k
            assert out["stats"]["hits"] == view["stats"]["hits"] == int(hit.sum()) and out["stats"]["samples"] == view["stats"]["samples"]
            assert out["stats"]["residual_sq_sum"] == 0.0
            assert np.array_equal(out["status"], np.where(hit, 3, 1))


def test_fusion_camera_rays_equal_the_fusion_renderer():
    sc = cases.scene()
    cam, o, d = cases.front_camera(sc)
    with _fusion(sc) as f:
        view = f.render(cam)
        out = f.cast_rays(o, d)
        assert set(out) == set(FUSION_ALL) | {"stats"}
        hit = view["depth"].ravel() > 0
        assert hit.sum() > 500
        assert np.array_equal(out["t"].astype(np.float32), view["depth"].ravel()) and np.array_equal(out["normal"], view["normal"].reshape(-1, 3))
        assert out["stats"] == view["stats"]
        assert np.array_equal(out["position"], np.where(hit[:, None], o + out["t"][:, None] * d, 0.0))
        _same(out, f.cast_rays(o, d, order=1), FUSION_ALL)


# ---- 2. against the twin on general rays -----------------------------------------------------------------------------------------------------------------------
def test_general_rays_match_the_twin(plain):
    """The bars of tests/test_gpu_render.py's _compare, t differences taken as world length |dt| |d|.  Measured on MI355X: 360 hits on both sides, no mask difference, every depth difference 0 (checks)."""
    g = plain["general"]; tw = plain["tw"]; vs = plain["grid"].vs
    o, d, lo, hi = plain["o"][g], plain["d"][g], plain["lo"][g], plain["hi"][g]
    dev = plain["ctx"].cast_rays(o, d, lo, hi, outputs=ALL)
    hd, ht = (dev["status"] & 2) != 0, tw["hit"]
    assert ht.sum() > 200
    print("hits device / twin", int(hd.sum()), int(ht.sum()), "mask differences", int((hd != ht).sum()))
    assert (hd != ht).sum() <= 0.002 * ht.sum(), ((hd & ~ht).sum(), (ht & ~hd).sum(), ht.sum())
    common = hd & ht
    length = np.sqrt((d * d).sum(1))
    dd = (np.abs(dev["t"] - tw["t"]) * length)[common]
    print("depth difference in voxels: q0.999", np.quantile(dd, 0.999) / vs, "max", dd.max() / vs)
    assert np.quantile(dd, 0.999) <= 1e-3 * vs and dd.max() <= 0.05 * vs, (np.quantile(dd, 0.999) / vs, dd.max() / vs)
    same = common & (np.abs(dev["t"] - tw["t"]) * length <= 1e-3 * vs)           # the rays whose march took the same path
    dot = np.clip((dev["normal"].astype(np.float64) * tw["normal"]).sum(-1), -1.0, 1.0)[same]
    assert np.arccos(dot).max() <= 1e-3
    for k in ("albedo", "shading", "intensity"):
        assert np.abs(dev[k] - tw[k])[same].max() <= 1e-4, k
    # position is o + t d exactly, the status bits agree with the outputs, every output of a ray without a hit is 0
    assert np.array_equal(dev["position"], np.where(hd[:, None], o + dev["t"][:, None] * d, 0.0))
    assert np.all(dev["status"] & 1) and np.array_equal(hd, dev["t"] != 0.0) and not np.any(dev["status"] & 4)
    for k in ("t", "position", "normal", "albedo", "shading", "intensity"):
        assert not np.any(dev[k][~hd]), k
    assert np.all(dev["t"][hd] >= lo[hd]) and np.all((dev["t"] < np.where(hi > 0, hi, np.inf))[hd])
    assert dev["stats"]["hits"] == int(hd.sum()) and dev["stats"]["residual_sq_sum"] == 0.0
    assert abs(dev["stats"]["samples"] - int(tw["samples"].sum())) <= 0.01 * tw["samples"].sum()


# ---- 3. order = 1 is order = 0 -----------------------------------------------------------------------------------------------------------------------------------
def _mixed(plain, seed=3):
    """the union of the camera's and the general rays under a seeded shuffle, invalid rays mixed in"""
    rng = np.random.default_rng(seed)
    io, idr, ilo, ihi = cases.invalid_rays(plain["grid"].vs)
    o = np.concatenate([plain["o"], io]); d = np.concatenate([plain["d"], idr])
    lo = np.concatenate([plain["lo"], ilo]); hi = np.concatenate([plain["hi"], ihi])
    p = rng.permutation(len(o))
    return o[p], d[p], lo[p], hi[p]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, None])
def test_coherent_order_changes_no_bit(plain, n):
    o, d, lo, hi = _mixed(plain)
    if n is None:
        n = len(o)
        assert n % 64 != 0 and n > 64 * 100
    ctx = plain["ctx"]
    a = ctx.cast_rays(o[:n], d[:n], lo[:n], hi[:n], outputs=ALL, order=0)
    b = ctx.cast_rays(o[:n], d[:n], lo[:n], hi[:n], outputs=ALL, order=1)
    _same(a, b, ALL)
    if n == 0:
        assert a["stats"] == dict(hits=0, samples=0, residual_sq_sum=0.0) and all(a[k].shape[0] == 0 for k in ALL)
    if n > 1000:
        assert a["stats"]["hits"] > 500 and (a["status"] == 0).sum() == 15
        only = ctx.cast_rays(o, d, lo, hi, outputs=("t",), order=1)                 # fewer outputs: the same values
        assert np.array_equal(only["t"], a["t"]) and only["stats"] == a["stats"] and set(only) == {"t", "stats"}


# ---- 4. invalid rays ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1])
def test_invalid_rays_are_not_marched(plain, order):
    """every way of being invalid scattered through a wave of valid rays: status 0 and zeros; the valid ones as in the run without them"""
    ctx = plain["ctx"]
    sel = np.arange(0, plain["n_cam"], 61)[:80]                                     # 80 valid rays: two waves, the second one part full
    o, d = plain["o"][sel], plain["d"][sel]
    alone = ctx.cast_rays(o, d, outputs=ALL, order=order)
    assert alone["stats"]["hits"] > 10
    io, idr, ilo, ihi = cases.invalid_rays(plain["grid"].vs)
    m = len(io)
    pos = np.linspace(0, len(o), m, endpoint=False).astype(int)
    ao = np.insert(o, pos, io, 0); ad = np.insert(d, pos, idr, 0)
    alo = np.insert(np.zeros(len(o)), pos, ilo); ahi = np.insert(np.zeros(len(o)), pos, ihi)
    bad = np.zeros(len(ao), bool); bad[pos + np.arange(m)] = True
    out = ctx.cast_rays(ao, ad, alo, ahi, outputs=ALL, order=order)
    for k in ALL:
        assert not np.any(out[k][bad]), k
        assert np.array_equal(out[k][~bad], alone[k]), k
    assert out["stats"] == alone["stats"]
    none = ctx.cast_rays(io, idr, ilo, ihi, outputs=ALL, order=order)
    assert none["stats"] == dict(hits=0, samples=0, residual_sq_sum=0.0) and not any(np.any(none[k]) for k in ALL)


# ---- 5. segments -------------------------------------------------------------------------------------------------------------------------------------------------
def test_segments(plain):
    """A -> B is occluded iff the ray (A, B - A, t_max = 1) hits: from the eye to 0.9 of the way to a hit point nothing, to 1.1 of the way the hit at t 1.1 = 1"""
    ctx = plain["ctx"]; vs = plain["grid"].vs
    o, d = plain["o"][:plain["n_cam"]], plain["d"][:plain["n_cam"]]
    first = ctx.cast_rays(o, d, outputs=("t", "position", "status"))
    hit = (first["status"] & 2) != 0
    assert hit.sum() > 500
    A = o[hit]; P = first["position"][hit]
    ones = np.ones(len(A))
    near = ctx.cast_rays(A, 0.9 * (P - A), None, ones, outputs=("t", "status"))
    assert near["stats"]["hits"] == 0 and np.all(near["status"] == 1)
    far = ctx.cast_rays(A, 1.1 * (P - A), None, ones, outputs=("t", "status"))
    assert np.all(far["status"] == 3)
    err = np.abs(far["t"] * 1.1 - 1.0) * np.linalg.norm(P - A, axis=1)              # world length
    print("segment depth difference in voxels: q0.999", np.quantile(err, 0.999) / vs, "max", err.max() / vs)
    assert np.quantile(err, 0.999) <= 1e-3 * vs and err.max() <= 0.05 * vs, (np.quantile(err, 0.999) / vs, err.max() / vs)


# ---- 6. changes nothing ------------------------------------------------------------------------------------------------------------------------------------------
def test_a_call_changes_nothing_in_the_context():
    sc = cases.scene()
    cam, o, d = cases.front_camera(sc)
    with _context(sc) as ctx:
        grid0, sh0 = ctx.export_grid(), ctx.get_voxel_sh()
        view0 = ctx.render_view(frame=-1, planes=PLANES, camera=cam)
        a = ctx.cast_rays(o, d, outputs=ALL, order=1)
        grid1, sh1 = ctx.export_grid(), ctx.get_voxel_sh()
        for k in grid0:
            assert np.array_equal(grid0[k], grid1[k]), k
        assert np.array_equal(sh0, sh1)
        view1 = ctx.render_view(frame=-1, planes=PLANES, camera=cam)
        for k in PLANES:
            assert np.array_equal(view0[k], view1[k]), k
        assert view0["stats"] == view1["stats"]
        # a change of the grid between two calls is seen by the second
        ctx.update_grid(sdf_refined=grid0["sdf_refined"] + 0.5 * float(sc["voxel_size"]))
        b = ctx.cast_rays(o, d, outputs=ALL, order=1)
        both = ((a["status"] & 2) != 0) & ((b["status"] & 2) != 0)
        assert both.sum() > 500 and np.all(b["t"][both] > a["t"][both])               # the surface moved inwards by half a voxel
        assert np.array_equal(b["t"].astype(np.float32), ctx.render_view(frame=-1, planes=("depth",), camera=cam)["depth"].ravel())


def test_a_call_changes_nothing_in_the_volume():
    sc = cases.scene()
    cam, o, d = cases.front_camera(sc)
    with _fusion(sc) as f:
        before = f.cast_rays(o, d, order=1)                                           # on the volume as it stands, before finish()
        assert before["stats"]["hits"] > 500
        get0, info0 = f.export(), f.info()
        a = f.cast_rays(o, d, order=0)
        get1, info1 = f.export(), f.info()
        assert info0 == info1
        for k in get0:
            assert np.array_equal(get0[k], get1[k]), k
        _same(a, f.cast_rays(o, d, order=1), FUSION_ALL)


# ---- 7. errors ---------------------------------------------------------------------------------------------------------------------------------------------------
INVALID, STATE, CAPACITY = 1, 4, 5
SENTINEL = -12345.0


class _Outs:
    """sentinel-filled outputs of one raw call and whether the call left them alone (the pattern of tests/test_gpu_model_errors.py)"""

    def __init__(self, n, names):
        shape = {"t": ((n,), np.float64), "position": ((n, 3), np.float64), "normal": ((n, 3), np.float32), "albedo": ((n,), np.float32),
                 "shading": ((n,), np.float32), "intensity": ((n,), np.float32), "status": ((n,), np.uint8)}
        self.a = {k: np.full(shape[k][0], 0xA5 if k == "status" else SENTINEL, shape[k][1]) for k in names}
        self.stats = binding.RenderStats(); C.memset(C.byref(self.stats), 0xA5, C.sizeof(self.stats))
        self.raw = [x.tobytes() for x in self.a.values()] + [bytes(self.stats)]

    def untouched(self):
        return [x.tobytes() for x in self.a.values()] + [bytes(self.stats)] == self.raw


def _raw(L, handle, fusion, n, o, d, order=0, want=None, null=False):
    """one raw call -> (code, outputs)"""
    names = FUSION_ALL if fusion else ALL
    outs = _Outs(max(int(n), 1) if 0 <= n <= 4 else 1, names)
    p = binding._p
    args = [p(outs.a[k]) if (want is None or k in want) else None for k in names]
    h = None if null else handle
    if fusion:
        rc = L.i3d_fusion_cast_rays(h, order, n, p(o), p(d), None, None, *args, C.byref(outs.stats))
    else:
        rc = L.i3d_cast_rays(h, 1, order, n, p(o), p(d), None, None, *args, C.byref(outs.stats))
    return rc, outs


def _argument_cases():
    o = np.zeros((1, 3)); d = np.array([[0.0, 0.0, 1.0]])
    return [("null handle", dict(n=1, o=o, d=d, null=True)), ("n negative", dict(n=-1, o=o, d=d)), ("n above 2^27", dict(n=(1 << 27) + 1, o=o, d=d)),
            ("null origins", dict(n=1, o=None, d=d)), ("null directions", dict(n=1, o=o, d=None)), ("order 2", dict(n=1, o=o, d=d, order=2)),
            ("order -1", dict(n=1, o=o, d=d, order=-1))]


def test_errors_of_the_context():
    L = binding.load()
    sc = cases.scene()
    name = "i3d_cast_rays"
    o = np.zeros((1, 3)); d = np.array([[0.0, 0.0, 1.0]])
    with binding.Context(0) as ctx:
        rc, outs = _raw(L, ctx.h, False, 1, o, d)
        assert rc == STATE and L.i3d_last_error(ctx.h).decode() == name + ": no grid" and outs.untouched()
        sdf_r, alb = cases.perturbed(sc)
        ctx.set_grid(sc["voxel_size"], sc["keys"], sc["sdf"], sdf_r, alb, sc["weight"], sc["color"])
        for what, kw in _argument_cases():
            rc, outs = _raw(L, ctx.h, False, **kw)
            assert rc == INVALID and outs.untouched(), what
            if not kw.get("null"):
                assert L.i3d_last_error(ctx.h).decode().startswith(name + ": "), what
        for want in (("shading",), ("intensity",), ("t", "shading", "intensity")):
            rc, outs = _raw(L, ctx.h, False, 1, o, d, want=want)
            assert rc == STATE and outs.untouched(), want
            assert L.i3d_last_error(ctx.h).decode() == name + ": shading and intensity need the per-voxel SH (i3d_set_voxel_sh / i3d_estimate_sh)"
        with pytest.raises(binding.I3DError, match=name):
            ctx.cast_rays(o, d, outputs=("shading",))
        with pytest.raises(ValueError):
            ctx.cast_rays(o, d, outputs=("depth",))
        with pytest.raises(ValueError):
            ctx.cast_rays(o, np.zeros((2, 3)))
        rc, outs = _raw(L, ctx.h, False, 0, None, None, want=("t", "albedo", "status"))      # n = 0: nothing but the stats, zeroed
        assert rc == 0 and bytes(outs.stats) == bytes(binding.RenderStats()) and [x.tobytes() for x in outs.a.values()] == outs.raw[:-1]
        rc, outs = _raw(L, ctx.h, False, 1, o, d, want=("t", "albedo", "status"))     # without SH everything else is served
        assert rc == 0 and outs.a["status"][0] == 1 and outs.a["shading"][0] == np.float32(SENTINEL)
    # the bitmap's capacity, as the renderer: two voxels whose bricks span more than 2^31 bits
    with binding.Context(0) as ctx:
        keys = np.array([[0, 0, 0], [16400, 16400, 16400]], np.int32)
        z = np.zeros(2)
        ctx.set_grid(sc["voxel_size"], keys, z, z, z + 0.5, np.ones(2, np.float32), np.zeros((2, 3), np.uint8))
        rc, outs = _raw(L, ctx.h, False, 1, o, d, want=("t", "status"))
        assert rc == CAPACITY and outs.untouched() and "would exceed 2^31 bits" in L.i3d_last_error(ctx.h).decode()


def test_errors_of_the_volume():
    L = binding.load()
    sc = cases.scene()
    name = "i3d_fusion_cast_rays"
    o = np.zeros((1, 3)); d = np.array([[0.0, 0.0, 1.0]])
    with binding.Fusion(float(sc["voxel_size"]), 0.01, 10.0, initial_capacity=1 << 16) as f:
        out = f.cast_rays(o, d)                                                       # an empty volume has no bricks: no hits
        assert out["stats"] == dict(hits=0, samples=0, residual_sq_sum=0.0) and out["status"][0] == 1
        for what, kw in _argument_cases():
            rc, outs = _raw(L, f.h, True, **kw)
            assert rc == INVALID and outs.untouched(), what
            if not kw.get("null"):
                assert L.i3d_fusion_last_error(f.h).decode().startswith(name + ": "), what
        rc, outs = _raw(L, f.h, True, 0, None, None)
        assert rc == 0 and bytes(outs.stats) == bytes(binding.RenderStats())
        # the bitmap's capacity: the same frame fused at two places 70 m apart on every axis
        fr = sc["frames"][0]; intr = sc["intr"].astype(np.float32)
        T = c2w(sc["poses"][0])
        f.integrate(fr["depth"][0], intr, fr["bgr"][0], intr, T, 2)
        assert f.cast_rays(o, d)["status"][0] == 1
        T2 = T.copy(); T2[:3, 3] += 70.0
        f.integrate(fr["depth"][0], intr, fr["bgr"][0], intr, T2, 2)
        rc, outs = _raw(L, f.h, True, 1, o, d)
        assert rc == CAPACITY and outs.untouched() and "would exceed 2^31 bits" in L.i3d_fusion_last_error(f.h).decode()
