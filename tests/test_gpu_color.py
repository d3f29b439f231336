"""The colour planes on the device: i3d_render_view_color / i3d_fusion_render_color / i3d_cast_rays_color / i3d_fusion_cast_rays_color.
The colour is albedo's interpolation bit for bit, a camera's rays equal its view, the fusion volume equals the context of its export, the general rays match
the numpy statement (color_twin.py), the coherent order changes no bit, a call changes nothing, and the fault table with nothing written."""
import ctypes as C

import numpy as np
import pytest

import cast_rays_cases as cases
import color_twin
import render_twin
from helpers import c2w
from intrinsic3d_amd import binding, synthetic

pytestmark = pytest.mark.gpu

ALL = binding.COLOR_CAST_OUTPUTS
ZERO_STATS = dict(hits=0, samples=0, residual_sq_sum=0.0)


def _random_colors(n, seed=35):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def _context(sc, keyframes=False):
    """the scene's grid (refined field and albedo perturbed) with seeded random colours set through update_grid; no per-voxel SH: the colour calls need none"""
    sdf_r, alb = cases.perturbed(sc)
    ctx = binding.Context(0)
    ctx.set_grid(sc["voxel_size"], sc["keys"], sc["sdf"], sdf_r, alb, sc["weight"], sc["color"])
    ctx.update_grid(color=_random_colors(ctx.N))
    if keyframes:
        ctx.set_frames(sc["frames"], sc["levels"])
        ctx.set_camera(sc["intr"], np.zeros(5), sc["poses"])
    return ctx


def _fuse(f, sc, keyframes=(0, 1, 2)):
    """the scene's textured keyframes and the front camera's view integrated into f"""
    for k in keyframes:
        _integrate_keyframe(f, sc, k)
    _integrate_front(f, sc)
    return f


def _integrate_keyframe(f, sc, k):
    intr = sc["intr"].astype(np.float32)
    fr = sc["frames"][k]
    f.integrate(fr["depth"][0], intr, fr["bgr"][0], intr, c2w(sc["poses"][k]), 2)


def _integrate_front(f, sc):
    cam = cases.front_camera(sc)[0]
    _, depth, bgr = synthetic.render_frame(sc["scene"], cam["pose"], cam["intr"], cam["width"], cam["height"])
    ci = cam["intr"].astype(np.float32)
    f.integrate(depth, ci, bgr, ci, c2w(cam["pose"]), 2)


def _volume(sc):
    return binding.Fusion(float(sc["voxel_size"]), 0.01, 10.0, initial_capacity=1 << 16)


def _rays(sc, per_kind=900):
    """the front camera, and the union of its rays and the general rays with their ranges (per_kind: general rays of each kind of origin; the volume fused from
    four views holds part of the surface, so its tests take twice as many to keep more than 200 hits)"""
    cam, co, cd = cases.front_camera(sc)
    go, gd, glo, ghi = cases.general_rays(sc, cases.cpu_grid(sc), per_kind=per_kind)
    o = np.concatenate([co, go]); d = np.concatenate([cd, gd])
    lo = np.concatenate([np.zeros(len(co)), glo]); hi = np.concatenate([np.zeros(len(co)), ghi])
    return cam, len(co), o, d, lo, hi


@pytest.fixture(scope="module")
def plain():
    """the scene at the origin, its context with random colours, the rays; shared, changed by no test"""
    sc = cases.scene()
    ctx = _context(sc)
    cam, n_cam, o, d, lo, hi = _rays(sc)
    yield dict(sc=sc, ctx=ctx, cam=cam, n_cam=n_cam, o=o, d=d, lo=lo, hi=hi)
    ctx.close()


def _same(a, b, names):
    for k in names:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    assert a["stats"] == b["stats"]


# ---- 1. the colour is albedo's interpolation, bit for bit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [None, cases.SHIFT], ids=["origin", "negative_octant"])
def test_colour_is_albedos_interpolation(shift):
    """with albedo := the stored byte of one channel, render_view's / cast_rays' albedo is that channel of the colour call, every bit; random unequal channels:
    a swapped channel or corner order fails here"""
    sc = cases.scene(shift=shift, levels=2)
    cam, n_cam, o, d, lo, hi = _rays(sc)
    views = [dict(frame=-1, camera=cam), dict(frame=0, level=1)]
    with _context(sc, keyframes=True) as ctx:
        color = ctx.export_grid()["color"]
        assert np.array_equal(color, _random_colors(ctx.N))                    # visit order in, visit order out
        col = {}
        for refined in (True, False):
            for i, v in enumerate(views):
                col[refined, i] = ctx.render_view_color(refined=refined, **v)
                hits = col[refined, i]["stats"]["hits"]
                print("view", i, "refined", refined, "hits", hits)
                assert hits > 500 and col[refined, i]["color"].dtype == np.float32 and col[refined, i]["stats"]["residual_sq_sum"] == 0.0
            col[refined, "rays"] = ctx.cast_rays_color(o, d, lo, hi, refined=refined)
            assert ((col[refined, "rays"]["status"][n_cam:] & 2) != 0).sum() > 200
        for ch in range(3):
            ctx.update_grid(albedo=color[:, ch].astype(np.float64))
            for refined in (True, False):
                for i, v in enumerate(views):
                    ref = ctx.render_view(refined=refined, planes=("depth", "albedo"), **v)
                    got = col[refined, i]
                    assert np.array_equal(ref["albedo"], got["color"][..., ch]), (ch, refined, i)
                    assert np.array_equal(ref["depth"], got["depth"]) and ref["stats"] == got["stats"]
                ref = ctx.cast_rays(o, d, lo, hi, outputs=("t", "albedo", "status"), refined=refined)
                got = col[refined, "rays"]
                assert np.array_equal(ref["albedo"], got["color"][:, ch]), (ch, refined)
                assert np.array_equal(ref["t"], got["t"]) and np.array_equal(ref["status"], got["status"]) and ref["stats"] == got["stats"]
                assert got["stats"]["residual_sq_sum"] == 0.0
        for refined in (True, False):                                            # the three channels differ: the planes are not grey
            c = col[refined, 0]["color"][col[refined, 0]["depth"] > 0]
            assert ((c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2])).mean() > 0.9
        assert not np.array_equal(col[True, 0]["depth"], col[False, 0]["depth"])           # use_refined_sdf chose the field that was marched
        # as_uint8 rounds the same floats on the host; a subset of the planes is the same values
        u8 = ctx.render_view_color(frame=-1, camera=cam, as_uint8=True)
        assert u8["color"].dtype == np.uint8 and np.array_equal(u8["color"], np.clip(np.rint(col[True, 0]["color"]), 0, 255).astype(np.uint8))
        only = ctx.render_view_color(frame=-1, camera=cam, planes=("color",))
        assert set(only) == {"color", "stats"} and np.array_equal(only["color"], col[True, 0]["color"]) and only["stats"] == col[True, 0]["stats"]


# ---- 2. a camera's rays equal its view ------------------------------------------------------------------------------------------------------------------------------
def test_camera_rays_equal_the_view(plain):
    ctx = plain["ctx"]; n = plain["n_cam"]
    o, d = plain["o"][:n], plain["d"][:n]
    for refined in (True, False):
        view = ctx.render_view_color(frame=-1, camera=plain["cam"], refined=refined)
        out = ctx.cast_rays_color(o, d, refined=refined)
        hit = view["depth"].ravel() > 0
        assert hit.sum() > 500
        assert np.array_equal(out["color"], view["color"].reshape(-1, 3)) and np.array_equal(out["t"].astype(np.float32), view["depth"].ravel())
        assert np.array_equal(out["status"], np.where(hit, 3, 1)) and out["stats"] == view["stats"]
        assert not np.any(out["color"][~hit]) and np.any(out["color"][hit])


def test_fusion_camera_rays_equal_the_fusion_view():
    sc = cases.scene()
    cam, o, d = cases.front_camera(sc)
    with _fuse(_volume(sc), sc) as f:
        view = f.render_color(cam)
        out = f.cast_rays_color(o, d)
        hit = view["depth"].ravel() > 0
        assert hit.sum() > 500
        assert np.array_equal(out["color"], view["color"].reshape(-1, 3)) and np.array_equal(out["t"].astype(np.float32), view["depth"].ravel())
        assert np.array_equal(out["status"], np.where(hit, 3, 1)) and out["stats"] == view["stats"]
        # depth, t, status and the stats are the siblings'
        sib = f.render(cam, planes=("depth",)); rays = f.cast_rays(o, d, outputs=("t", "status"))
        assert np.array_equal(sib["depth"], view["depth"]) and sib["stats"] == view["stats"]
        assert np.array_equal(rays["t"], out["t"]) and np.array_equal(rays["status"], out["status"]) and rays["stats"] == out["stats"]
        _same(out, f.cast_rays_color(o, d, order=1), ALL)


# ---- 3. the fusion volume equals the context of its export ------------------------------------------------------------------------------------------------------
def _volume_calls(f, cam, o, d, lo, hi):
    return f.render_color(cam), f.cast_rays_color(o, d, lo, hi)


def _context_calls(ex, vs, cam, o, d, lo, hi):
    with binding.Context(0) as ctx:
        s = ex["sdf"].astype(np.float64)
        ctx.set_grid(vs, ex["keys"], s, s, np.zeros_like(s), ex["weight"], ex["color"])
        return ctx.render_view_color(frame=-1, camera=cam, refined=False), ctx.cast_rays_color(o, d, lo, hi, refined=False)


def _distinct_in_hit_cells(ex, vs, o, d, lo, hi):
    """per channel, the number of distinct stored bytes among the corners of the cells the rays hit (from the numpy statement on the exported records)"""
    hit, corners = color_twin.hit_cells(render_twin.Grid(ex["keys"], ex["sdf"].astype(np.float64), ex["weight"], vs), o, d, lo, hi)
    corners = np.unique(corners[hit])
    return [len(np.unique(ex["color"][corners, ch])) for ch in range(3)]


def _equal_views(a, b):
    (va, ra), (vb, rb) = a, b
    _same(va, vb, ("color", "depth")); _same(ra, rb, ALL)


def test_fusion_equals_the_context_of_its_export():
    sc = cases.scene()
    vs = float(sc["voxel_size"])
    cam, n_cam, o, d, lo, hi = _rays(sc, per_kind=1800)
    # the colours as fused from the textured frames
    with _fuse(_volume(sc), sc) as f:
        before = _volume_calls(f, cam, o, d, lo, hi)
        assert before[0]["stats"]["hits"] > 500 and ((before[1]["status"][n_cam:] & 2) != 0).sum() > 200
        f.finish(0)
        ex = f.export()
        _equal_views(before, _volume_calls(f, cam, o, d, lo, hi))               # finish(0) leaves the table as it was
    _equal_views(before, _context_calls(ex, vs, cam, o, d, lo, hi))
    print("distinct stored bytes per channel in the hit cells, fused texture:", _distinct_in_hit_cells(ex, vs, o, d, lo, hi))
    # the same volume with seeded random colours poked into every stored voxel, sdf and weight kept: unequal channels whatever the texture gives
    rnd = dict(ex, color=_random_colors(len(ex["sdf"]), seed=36))
    distinct = _distinct_in_hit_cells(rnd, vs, o, d, lo, hi)
    print("distinct stored bytes per channel in the hit cells, poked:", distinct)
    assert min(distinct) >= 64
    with _fuse(_volume(sc), sc) as f:
        assert f.debug_poke_voxels(ex["keys"], ex["sdf"], ex["weight"], rnd["color"]).all()
        poked = _volume_calls(f, cam, o, d, lo, hi)
        f.finish(0)
        ex2 = f.export()
        _equal_views(poked, _volume_calls(f, cam, o, d, lo, hi))
    assert all(np.array_equal(ex2[k], rnd[k]) for k in ("keys", "sdf", "weight", "color"))
    _equal_views(poked, _context_calls(rnd, vs, cam, o, d, lo, hi))
    assert np.array_equal(poked[0]["depth"], before[0]["depth"]) and not np.array_equal(poked[0]["color"], before[0]["color"])


# ---- 4. against the numpy statement, general rays -------------------------------------------------------------------------------------------------------------
def test_general_rays_match_the_twin(plain):
    """The comparison of test_gpu_cast_rays.test_general_rays_match_the_twin; on the rays whose march took the same path |colour - twin| <= 255 x 1e-4, that test's
    albedo bar times the channel's range.  Measured on MI355X: see DESIGN.md section 35, checks."""
    ctx = plain["ctx"]; n = plain["n_cam"]
    o, d, lo, hi = plain["o"][n:], plain["d"][n:], plain["lo"][n:], plain["hi"][n:]
    a = ctx.export_grid()
    _, vs, _ = ctx.grid_info()
    grid = render_twin.Grid(a["keys"], a["sdf_refined"], a["weight"], vs)
    tw = color_twin.cast(grid, a["color"], o, d, lo, hi)
    dev = ctx.cast_rays_color(o, d, lo, hi)
    hd, ht = (dev["status"] & 2) != 0, tw["hit"]
    assert ht.sum() > 200
    print("hits device / twin", int(hd.sum()), int(ht.sum()), "mask differences", int((hd != ht).sum()))
    assert (hd != ht).sum() <= 0.002 * ht.sum(), ((hd & ~ht).sum(), (ht & ~hd).sum(), ht.sum())
    common = hd & ht
    length = np.sqrt((d * d).sum(1))
    same = common & (np.abs(dev["t"] - tw["t"]) * length <= 1e-3 * grid.vs)            # the rays whose march took the same path
    assert same.sum() > 200
    err = np.abs(dev["color"].astype(np.float64) - tw["color"])[same]
    print("rays on the same path", int(same.sum()), "of", int(common.sum()), "max |colour - twin|", err.max(), "bar", 255 * 1e-4)
    assert err.max() <= 255 * 1e-4
    exact = common & (dev["t"] == tw["t"])                   # the same t: the same cell, weights and fp64 sum, so the float rounding of the same double
    print("rays with the twin's t bit for bit", int(exact.sum()))
    assert np.array_equal(dev["color"][exact], tw["color"][exact].astype(np.float32))
    assert not np.any(dev["color"][~hd]) and not np.any(dev["t"][~hd]) and np.all(dev["status"] & 1)
    assert dev["stats"]["hits"] == int(hd.sum()) and dev["stats"]["residual_sq_sum"] == 0.0


# ---- 5. order = 1 changes no bit --------------------------------------------------------------------------------------------------------------------------------
def _mixed(plain, seed=3):
    """the union of the camera's and the general rays under a seeded shuffle, invalid rays mixed in"""
    rng = np.random.default_rng(seed)
    io, idr, ilo, ihi = cases.invalid_rays(float(np.float32(plain["sc"]["voxel_size"])))
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
    a = ctx.cast_rays_color(o[:n], d[:n], lo[:n], hi[:n], order=0)
    b = ctx.cast_rays_color(o[:n], d[:n], lo[:n], hi[:n], order=1)
    _same(a, b, ALL)
    assert a["color"].shape == (n, 3) and a["t"].shape == (n,) and a["status"].shape == (n,)
    if n == 0:
        assert a["stats"] == ZERO_STATS
    invalid = a["status"] == 0; miss = (a["status"] & 2) == 0
    assert not np.any(a["t"][miss]) and not np.any(a["color"][miss]) and np.all(a["status"][invalid] == 0)
    if n > 1000:
        assert a["stats"]["hits"] > 500 and invalid.sum() == 15
        only = ctx.cast_rays_color(o, d, lo, hi, outputs=("color",), order=1)            # fewer outputs: the same values
        assert np.array_equal(only["color"], a["color"]) and only["stats"] == a["stats"] and set(only) == {"color", "stats"}
        sib = ctx.cast_rays(o, d, lo, hi, outputs=("t", "status"), order=1)              # t, status and the stats are the sibling's
        assert np.array_equal(sib["t"], a["t"]) and np.array_equal(sib["status"], a["status"]) and sib["stats"] == a["stats"]


# ---- 6. a call changes nothing ------------------------------------------------------------------------------------------------------------------------------------
def test_a_call_changes_nothing_in_the_context():
    sc = cases.scene(levels=2)
    cam, n_cam, o, d, lo, hi = _rays(sc)
    planes = ("depth", "normal", "albedo", "shading", "intensity")
    with _context(sc, keyframes=True) as ctx:
        ctx.set_voxel_sh(np.tile(synthetic.SH_TRUE, (ctx.N, 1)))
        grid0, sh0, cam0 = ctx.export_grid(), ctx.get_voxel_sh(), ctx.get_camera()
        view0 = ctx.render_view(frame=-1, planes=planes, camera=cam)
        key0 = ctx.render_view(frame=0, level=1)
        rays0 = ctx.cast_rays(o, d, lo, hi, outputs=binding.CAST_OUTPUTS, order=1)
        q0 = ctx.query_points(o[:64] + d[:64] * 0.16)
        c0 = (ctx.render_view_color(frame=-1, camera=cam), ctx.render_view_color(frame=0, level=1), ctx.cast_rays_color(o, d, lo, hi, order=1),
              ctx.cast_rays_color(o, d, lo, hi, refined=False))
        assert c0[0]["stats"]["hits"] > 500 and c0[1]["stats"]["hits"] > 500
        grid1, sh1, cam1 = ctx.export_grid(), ctx.get_voxel_sh(), ctx.get_camera()
        for k in grid0:
            assert np.array_equal(grid0[k], grid1[k]), k
        assert np.array_equal(sh0, sh1) and all(np.array_equal(x, y) for x, y in zip(cam0, cam1))
        view1 = ctx.render_view(frame=-1, planes=planes, camera=cam)
        _same(view0, view1, planes)
        _same(key0, ctx.render_view(frame=0, level=1), binding.RENDER_PLANES)
        _same(rays0, ctx.cast_rays(o, d, lo, hi, outputs=binding.CAST_OUTPUTS, order=1), binding.CAST_OUTPUTS)
        _same(q0, ctx.query_points(o[:64] + d[:64] * 0.16), [k for k in q0 if k != "stats"])
        # a colour set between two calls is seen by the second; the field's outputs stay
        ctx.update_grid(color=_random_colors(ctx.N, seed=37))
        c1 = ctx.render_view_color(frame=-1, camera=cam)
        assert np.array_equal(c1["depth"], c0[0]["depth"]) and c1["stats"] == c0[0]["stats"] and not np.array_equal(c1["color"], c0[0]["color"])


def test_a_call_changes_nothing_in_the_volume():
    sc = cases.scene()
    cam, n_cam, o, d, lo, hi = _rays(sc)
    with _fuse(_volume(sc), sc, keyframes=(1, 2)) as f, _fuse(_volume(sc), sc, keyframes=(1, 2)) as fresh:
        view0, rays0 = f.render(cam), f.cast_rays(o, d, lo, hi, order=1)
        q0 = f.query_points(o[:64] + d[:64] * 0.16)
        info0 = f.info()
        a = _volume_calls(f, cam, o, d, lo, hi)                                  # on the volume as it stands, before finish()
        assert a[0]["stats"]["hits"] > 500
        assert f.info() == info0
        _same(view0, f.render(cam), ("depth", "normal")); _same(rays0, f.cast_rays(o, d, lo, hi, order=1), ("t", "position", "normal", "status"))
        _same(q0, f.query_points(o[:64] + d[:64] * 0.16), [k for k in q0 if k != "stats"])
        # an integrate afterwards gives what a fresh volume gives
        _integrate_keyframe(f, sc, 0); _integrate_keyframe(fresh, sc, 0)
        b = _volume_calls(f, cam, o, d, lo, hi)
        _equal_views(b, _volume_calls(fresh, cam, o, d, lo, hi))                 # the bitmap and the colours follow the table
        f.finish(0); fresh.finish(0)
        get0, want = f.export(), fresh.export()
        for k in want:
            assert np.array_equal(get0[k], want[k]), k
        _equal_views(b, _volume_calls(f, cam, o, d, lo, hi))
        get1 = f.export()
        for k in get0:
            assert np.array_equal(get0[k], get1[k]), k


# ---- 7. errors, with nothing written --------------------------------------------------------------------------------------------------------------------------------
INVALID, STATE = 1, 4
SENTINEL = -12345.0
p = binding._p


class _Outs:
    """sentinel-filled outputs of one raw call and whether the call left them alone"""

    def __init__(self):
        self.color = np.full((4, 4, 3), SENTINEL, np.float32); self.depth = np.full((4, 4), SENTINEL, np.float32)
        self.t = np.full(16, SENTINEL, np.float64); self.status = np.full(16, 0xA5, np.uint8)
        self.stats = binding.RenderStats(); C.memset(C.byref(self.stats), 0xA5, C.sizeof(self.stats))
        self.raw = self._bytes()

    def _bytes(self):
        return [x.tobytes() for x in (self.color, self.depth, self.t, self.status)] + [bytes(self.stats)]

    def untouched(self):
        return self._bytes() == self.raw


def _view(L, fusion, h, desc):
    outs = _Outs()
    fn = L.i3d_fusion_render_color if fusion else L.i3d_render_view_color
    return fn(h, None if desc is None else C.byref(desc), p(outs.color), p(outs.depth), C.byref(outs.stats)), outs


def _cast(L, fusion, h, n, o, d, order=0):
    outs = _Outs()
    tail = (n, p(o), p(d), None, None, p(outs.t), p(outs.color), p(outs.status), C.byref(outs.stats))
    rc = L.i3d_fusion_cast_rays_color(h, order, *tail) if fusion else L.i3d_cast_rays_color(h, 1, order, *tail)
    return rc, outs


CAM = dict(width=4, height=4, intr=[30.0, 30.0, 1.5, 1.5], dist=np.zeros(5), pose=np.zeros(6))
O1 = np.zeros((1, 3)); D1 = np.array([[0.0, 0.0, 1.0]])
CAST_FAULTS = [("n negative", dict(n=-1, o=O1, d=D1)), ("n above 2^27", dict(n=(1 << 27) + 1, o=O1, d=D1)), ("null origins", dict(n=1, o=None, d=D1)),
               ("null directions", dict(n=1, o=O1, d=None)), ("order 2", dict(n=1, o=O1, d=D1, order=2)), ("order -1", dict(n=1, o=O1, d=D1, order=-1))]


def test_errors_of_the_context():
    L = binding.load()
    sc = cases.scene()
    free = binding._render_desc(CAM, None)
    for fn, call in (("i3d_render_view_color", lambda h: _view(L, False, h, free)), ("i3d_cast_rays_color", lambda h: _cast(L, False, h, 1, O1, D1))):
        rc, outs = call(None)
        assert rc == INVALID and outs.untouched(), fn
    with binding.Context(0) as ctx:
        rc, outs = _view(L, False, ctx.h, free)
        assert rc == STATE and L.i3d_last_error(ctx.h).decode() == "i3d_render_view_color: no grid" and outs.untouched()
        rc, outs = _cast(L, False, ctx.h, 1, O1, D1)
        assert rc == STATE and L.i3d_last_error(ctx.h).decode() == "i3d_cast_rays_color: no grid" and outs.untouched()
        sdf_r, alb = cases.perturbed(sc)
        ctx.set_grid(sc["voxel_size"], sc["keys"], sc["sdf"], sdf_r, alb, sc["weight"], sc["color"])
        rc, outs = _view(L, False, ctx.h, None)
        assert rc == INVALID and outs.untouched() and L.i3d_last_error(ctx.h).decode() == "i3d_render_view_color: null argument"
        for what, desc in (("width 0", binding._render_desc(dict(CAM, width=0), None)), ("height too large", binding._render_desc(dict(CAM, height=32769), None))):
            rc, outs = _view(L, False, ctx.h, desc)
            assert rc == INVALID and outs.untouched() and L.i3d_last_error(ctx.h).decode() == "i3d_render_view_color: image size out of range", what
        for what, kw in CAST_FAULTS:
            rc, outs = _cast(L, False, ctx.h, **kw)
            assert rc == INVALID and outs.untouched() and L.i3d_last_error(ctx.h).decode().startswith("i3d_cast_rays_color: "), what
        # no per-voxel SH is present: not an error, for either call
        rc, outs = _view(L, False, ctx.h, free)
        assert rc == 0 and not outs.untouched() and outs.stats.samples >= 0 and outs.stats.residual_sq_sum == 0.0
        rc, outs = _cast(L, False, ctx.h, 1, O1, D1)
        assert rc == 0 and outs.status[0] == 1 and outs.t[0] == 0.0 and not np.any(outs.color[0, 0]) and outs.t[1] == SENTINEL and outs.status[1] == 0xA5
        # n = 0: nothing but the stats, zeroed
        rc, outs = _cast(L, False, ctx.h, 0, None, None)
        assert rc == 0 and bytes(outs.stats) == bytes(binding.RenderStats()) and outs._bytes()[:-1] == outs.raw[:-1]
        # every output may be NULL
        assert L.i3d_render_view_color(ctx.h, C.byref(free), None, None, None) == 0
        assert L.i3d_cast_rays_color(ctx.h, 1, 0, 1, p(O1), p(D1), None, None, None, None, None, None) == 0
        with pytest.raises(ValueError):
            ctx.render_view_color(frame=-1, camera=CAM, planes=("albedo",))
        with pytest.raises(ValueError):
            ctx.cast_rays_color(O1, D1, outputs=("position",))


def test_errors_of_the_volume():
    L = binding.load()
    sc = cases.scene()
    free = binding._render_desc(CAM, None)
    for fn, call in (("i3d_fusion_render_color", lambda h: _view(L, True, h, free)), ("i3d_fusion_cast_rays_color", lambda h: _cast(L, True, h, 1, O1, D1))):
        rc, outs = call(None)
        assert rc == INVALID and outs.untouched(), fn
    with _volume(sc) as f:
        out = f.cast_rays_color(O1, D1)                                              # an empty volume has no bricks: no hits, black
        assert out["stats"] == ZERO_STATS and out["status"][0] == 1 and not np.any(out["color"])
        view = f.render_color(CAM)
        assert view["stats"]["hits"] == 0 and not np.any(view["color"]) and not np.any(view["depth"])
        rc, outs = _view(L, True, f.h, None)
        assert rc == INVALID and outs.untouched() and L.i3d_fusion_last_error(f.h).decode() == "i3d_fusion_render_color: null descriptor"
        for what, desc in (("frame 0", binding._render_desc(None, None, 0, 0)), ("frame 3 with a camera", binding._render_desc(CAM, None, 3)),
                           ("frame -2", binding._render_desc(CAM, None, -2))):
            rc, outs = _view(L, True, f.h, desc)
            assert rc == INVALID and outs.untouched(), what
            assert L.i3d_fusion_last_error(f.h).decode() == "i3d_fusion_render_color: desc->frame must be -1 (a free camera; the volume has no keyframes)", what
        rc, outs = _view(L, True, f.h, binding._render_desc(dict(CAM, width=0), None))
        assert rc == INVALID and outs.untouched() and "image size" in L.i3d_fusion_last_error(f.h).decode()
        for what, kw in CAST_FAULTS:
            rc, outs = _cast(L, True, f.h, **kw)
            assert rc == INVALID and outs.untouched() and L.i3d_fusion_last_error(f.h).decode().startswith("i3d_fusion_cast_rays_color: "), what
        rc, outs = _cast(L, True, f.h, 0, None, None)
        assert rc == 0 and bytes(outs.stats) == bytes(binding.RenderStats()) and outs._bytes()[:-1] == outs.raw[:-1]
        with pytest.raises(ValueError, match="depth and normal only"):                # Fusion.render keeps its planes and its message
            f.render(CAM, planes=("color",))
