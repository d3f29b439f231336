"""numpy statement of the colour at a hit: i3d_render_view_color / i3d_fusion_render_color / i3d_cast_rays_color /
i3d_fusion_cast_rays_color, in fp64.

Test infrastructure: the colour kernels are compared against this.  No march of its own: cast_rays_twin.cast and render_twin.render already return
albedo = _tri(w, g.alb[c]) in the cell the hit's attributes are taken in, and channel ch of the colour is that output of a Grid whose albedo is the stored byte of
channel ch widened to fp64 - the same weights, the same sum, the same cell.  So the statement is three calls of the existing twin, one per channel R, G, B.
The corners of that cell (which neither twin returns) are read off the grid's own lookups: both twins end with the cell of t_hit and then the cell of the hit
sample, and take the second where the first is not valid.
"""
from __future__ import annotations

import numpy as np

import cast_rays_twin
import render_twin


class _Recording(render_twin.Grid):
    """a Grid that keeps (corners, valid) of every cell lookup a twin makes on it"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.lookups = []

    def cell(self, b):
        c, v, ok = super().cell(b)
        self.lookups.append((c, ok))
        return c, v, ok


def channel_grids(grid: render_twin.Grid, color):
    """the three grids of the statement: grid's voxels, field and weights with albedo = color[:, ch] as float64 and no SH; the first records its lookups"""
    color = np.asarray(color)
    assert color.dtype == np.uint8 and color.shape == (grid.keys.shape[0], 3)
    return [(_Recording if ch == 0 else render_twin.Grid)(grid.keys, grid.sdf, grid.weight, grid.vs, albedo=color[:, ch].astype(np.float64)) for ch in range(3)]


def _corners(rec, hit):
    """[n, 8] voxel indices of the cell the colour was taken in, -1 for a ray without a hit: the last two lookups are t_hit's cell and the hit sample's"""
    (c, ok), (cb, _) = rec.lookups[-2], rec.lookups[-1]
    out = np.full((hit.size, 8), -1, np.int64)
    out[np.nonzero(hit.ravel())[0]] = np.where(ok[:, None], c, cb)
    return out


def hit_cells(grid: render_twin.Grid, origins, dirs, t_min=None, t_max=None):
    """(hit [n], corners [n, 8]) of the rays alone: one march, no colour"""
    rec = _Recording(grid.keys, grid.sdf, grid.weight, grid.vs)
    out = cast_rays_twin.cast(rec, origins, dirs, t_min, t_max)
    return out["hit"], _corners(rec, out["hit"])


def cast(grid: render_twin.Grid, color, origins, dirs, t_min=None, t_max=None):
    """cast_rays_twin.cast's valid, hit, samples, status and t, with color [n, 3] float64 (R, G, B in units of the stored byte, 0 without a hit) and corners [n, 8]"""
    gs = channel_grids(grid, color)
    outs = [cast_rays_twin.cast(g, origins, dirs, t_min, t_max) for g in gs]
    for o in outs[1:]:                                # the march reads no albedo: the three calls walked the same path
        assert np.array_equal(o["t"], outs[0]["t"]) and np.array_equal(o["status"], outs[0]["status"])
    res = {k: outs[0][k] for k in ("valid", "hit", "samples", "status", "t")}
    res["color"] = np.stack([o["albedo"] for o in outs], -1)
    res["corners"] = _corners(gs[0], res["hit"])
    return res


def render(grid: render_twin.Grid, color, cam, tmin=0.0, tmax=0.0):
    """render_twin.render's hit, samples and depth over (h, w), with color (h, w, 3) float64 and corners (h, w, 8)"""
    gs = channel_grids(grid, color)
    outs = [render_twin.render(g, cam, tmin, tmax) for g in gs]
    for o in outs[1:]:
        assert np.array_equal(o["depth"], outs[0]["depth"])
    res = {k: outs[0][k] for k in ("hit", "samples", "depth")}
    res["color"] = np.stack([o["albedo"] for o in outs], -1)
    res["corners"] = _corners(gs[0], res["hit"]).reshape(cam["h"], cam["w"], 8)
    return res
