"""-m "not gpu": the four colour entry points in the header, the ABI table and the binding; the struct set they must not widen; and the
numpy statement of the colour (color_twin.py) on the scene of cast_rays_cases with seeded random bytes per voxel and channel."""
import os
import re

import numpy as np
import pytest

import cast_rays_cases as cases
import color_twin
import render_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NAMES = ("i3d_render_view_color", "i3d_fusion_render_color", "i3d_cast_rays_color", "i3d_fusion_cast_rays_color")


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "intrinsic3d_hip.h")).read(), flags=re.S)


def test_entry_points_are_declared_and_bound():
    from intrinsic3d_amd import abi, binding
    hdr = _header()
    table = {n: (r, a) for n, r, a in abi.PROTOTYPES}
    for name in NAMES:
        assert name in table and name in binding.EXPORTS and re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert table[name][0] is abi.i32 and table[name][1][-1]._type_ is abi.RenderStats, name
    # plain parameters: (handle, descriptor, color, depth, stats) and (handle, [use_refined_sdf,] order, n, 4 inputs, t, color, status, stats)
    assert [len(table[n][1]) for n in NAMES] == [5, 5, 12, 11]
    assert table["i3d_cast_rays_color"][1][1:4] == [abi.i32, abi.i32, abi.i64] and table["i3d_fusion_cast_rays_color"][1][1:3] == [abi.i32, abi.i64]
    for cls, methods in ((binding.Context, ("render_view_color", "cast_rays_color")), (binding.Fusion, ("render_color", "cast_rays_color"))):
        for m in methods:
            assert callable(getattr(cls, m)), (cls, m)
    assert binding.COLOR_CAST_OUTPUTS == ("t", "color", "status")


def test_header_struct_set_is_still_the_25_mirrors():
    """the colour entry points use plain parameters and bring no struct"""
    import ctypes
    from intrinsic3d_amd import abi
    declared = set(re.findall(r"\}\s*(i3d_[a-z0-9_]+)\s*;", _header())) - {"i3d_status"}
    mirrors = {v._c_name_ for v in vars(abi).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and "_c_name_" in vars(v)}
    assert mirrors == declared - {"i3d_lm_record"} and len(mirrors) == 25


def test_as_uint8_rounds_to_nearest_and_clips():
    from intrinsic3d_amd import binding
    out = binding._color_out({"color": np.array([[-0.2, 0.49, 0.51], [254.5, 255.4, 300.0], [1.5, 2.5, 127.5]], np.float32), "t": np.zeros(3)}, True)
    assert out["color"].dtype == np.uint8 and out["color"].tolist() == [[0, 0, 1], [254, 255, 255], [2, 2, 128]]         # rint: ties to even
    keep = np.ones((2, 3), np.float32)
    assert binding._color_out({"color": keep}, False)["color"] is keep and binding._color_out({"t": keep}, True) == {"t": keep}


@pytest.fixture(scope="module")
def scene():
    sc = cases.scene()
    grid = cases.cpu_grid(sc)
    color = np.random.default_rng(35).integers(0, 256, (sc["keys"].shape[0], 3), dtype=np.uint8)
    cam, o, d = cases.front_camera(sc)
    return dict(sc=sc, grid=grid, color=color, cam=cam, o=o, d=d, view=color_twin.cast(grid, color, o, d))


def _inside_corner_range(col, corners, color):
    """every channel within [min, max] of the eight corner bytes, up to one float ulp"""
    c32 = col.astype(np.float32)
    cb = color[corners].astype(np.float32)                       # [m, 8, 3]
    lo = np.nextafter(cb.min(1), np.float32(-np.inf)); hi = np.nextafter(cb.max(1), np.float32(np.inf))
    return bool(np.all(c32 >= lo) and np.all(c32 <= hi))


def test_twin_colour_properties(scene):
    out = scene["view"]; color = scene["color"]
    hit = out["hit"]
    assert hit.sum() > 500
    assert not np.any(out["color"][~hit]) and np.all(out["corners"][~hit] == -1)
    assert np.all(out["corners"][hit] >= 0)
    assert _inside_corner_range(out["color"][hit], out["corners"][hit], color)
    c = out["color"][hit]
    distinct = (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2])
    assert distinct.mean() > 0.9, distinct.mean()
    # the same on the general rays with ranges, and on invalid rays: nothing marched, nothing coloured
    go, gd, glo, ghi = cases.general_rays(scene["sc"], scene["grid"])
    gen = color_twin.cast(scene["grid"], color, go, gd, glo, ghi)
    gh = gen["hit"]
    assert gh.sum() > 200 and not np.any(gen["color"][~gh])
    assert _inside_corner_range(gen["color"][gh], gen["corners"][gh], color)
    io, idr, ilo, ihi = cases.invalid_rays(scene["grid"].vs)
    bad = color_twin.cast(scene["grid"], color, io, idr, ilo, ihi)
    assert not bad["valid"].any() and not np.any(bad["color"]) and not np.any(bad["status"])


def test_twin_is_the_trilinear_sum_of_the_corner_bytes(scene):
    """the statement spelled out once, independently of the twins' _tri: at the hit position q = (o + t d) / vs in the recorded cell, per channel the sum over the
    eight corners of weight x byte agrees to rounding (the cell's base is its corner 0)"""
    out = scene["view"]; g = scene["grid"]; hit = out["hit"]
    q = (scene["o"][hit] + out["t"][hit, None] * scene["d"][hit]) / g.vs
    f = q - g.keys[out["corners"][hit][:, 0]]
    assert np.all(f > -1e-9) and np.all(f < 1.0 + 1e-9)
    ref = np.zeros((hit.sum(), 3))
    for i in range(8):
        w = np.prod(np.where(np.array([i & 1, (i >> 1) & 1, i >> 2], bool), f, 1.0 - f), axis=1)
        ref += w[:, None] * scene["color"][out["corners"][hit][:, i]].astype(np.float64)
    assert np.abs(ref - out["color"][hit]).max() < 1e-9


def test_ray_twin_equals_the_view_twin(scene):
    """fed the camera's rays, the statement for rays is the statement for views, exactly"""
    cam = scene["cam"]
    rcam = render_twin.camera_from_pose(cam["pose"], cam["intr"], cam["dist"], cam["width"], cam["height"])
    d, _ = render_twin.rays(rcam)
    assert np.array_equal(d, scene["d"]) and np.array_equal(np.broadcast_to(rcam["eye"], d.shape), scene["o"])
    view = color_twin.render(scene["grid"], scene["color"], rcam)
    out = scene["view"]
    assert np.array_equal(view["hit"].ravel(), out["hit"]) and np.array_equal(view["depth"].ravel(), out["t"])
    assert np.array_equal(view["color"].reshape(-1, 3), out["color"]) and np.array_equal(view["corners"].reshape(-1, 8), out["corners"])
    assert np.array_equal(view["samples"].ravel(), out["samples"])
