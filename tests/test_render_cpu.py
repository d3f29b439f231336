"""i3d_render_view without a device: the ctypes mirrors of its structs, and the numpy statement of the renderer (render_twin.py) against an analytic sphere."""
import os
import subprocess
import tempfile

import numpy as np

import render_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_struct_layouts_match_header():
    import ctypes
    from intrinsic3d_amd import binding
    src = '#include <stdio.h>\n#include "intrinsic3d_hip.h"\nint main(){printf("%zu %zu\\n", sizeof(i3d_render_desc), sizeof(i3d_render_stats));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        sizes = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    assert sizes == [ctypes.sizeof(binding.RenderDesc), ctypes.sizeof(binding.RenderStats)]
    assert "i3d_render_view" in binding.EXPORTS


def _sphere_grid(vs=0.004, R_vox=12.0, center_key=(37.3, -21.6, 8.2), band=3.0):
    c = np.asarray(center_key) * vs
    lo = np.floor(np.asarray(center_key) - R_vox - band - 2).astype(int); hi = np.ceil(np.asarray(center_key) + R_vox + band + 2).astype(int)
    g = np.stack(np.meshgrid(*[np.arange(lo[a], hi[a]) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    sdf = np.sqrt(((g * vs - c) ** 2).sum(1)) - R_vox * vs
    keep = np.abs(sdf) <= band * vs
    keys = g[keep].astype(np.int32)
    rng = np.random.default_rng(0)
    perm = rng.permutation(keys.shape[0])                  # any visit order
    return keys[perm], sdf[keep][perm], c, R_vox * vs


def _erode(m, r):
    out = m.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out &= np.roll(np.roll(m, dy, 0), dx, 1)
    return out


def test_twin_against_analytic_sphere():
    from intrinsic3d_amd import synthetic
    vs = float(np.float32(0.004))
    keys, sdf, c, R = _sphere_grid(vs=vs)
    n = keys.shape[0]
    alb = np.full(n, 0.7); sh = np.tile(synthetic.SH_TRUE, (n, 1))
    grid = render_twin.Grid(keys, sdf, np.ones(n, np.float32), vs, albedo=alb, sh=sh)
    w, h = 64, 48
    intr = np.array([70.0, 70.0, (w - 1) * 0.5, (h - 1) * 0.5])
    for k, eye_dir in enumerate(([0.3, 0.5, -1.0], [-1.0, 0.2, 0.4], [0.1, -1.0, 0.2])):
        e = np.asarray(eye_dir) / np.linalg.norm(eye_dir)
        pose = synthetic.look_at_pose(c + 3.5 * R * e, c)
        dist = np.zeros(5) if k < 2 else np.array([0.04, -0.01, 0.002, 0.001, -0.0015])
        cam = render_twin.camera_from_pose(pose, intr, dist, w, h)
        out = render_twin.render(grid, cam)
        # analytic intersection of the same rays with the sphere (t = camera z)
        d = out["dir"].reshape(-1, 3); oc = cam["eye"] - c
        a = (d * d).sum(1); b = 2.0 * (d @ oc); cc = oc @ oc - R * R
        disc = b * b - 4 * a * cc
        ref_hit = (disc > 0).reshape(h, w)
        t_ref = ((-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)).reshape(h, w)
        inner = _erode(ref_hit, 2) & _erode(out["hit"], 2)
        assert inner.sum() > 0.2 * w * h
        assert (out["hit"] == ref_hit).mean() > 0.97
        dd = np.abs(out["depth"] - t_ref)[inner]
        assert np.median(dd) <= 0.05 * vs and dd.max() <= 0.5 * vs, (np.median(dd) / vs, dd.max() / vs)
        p = cam["eye"] + t_ref[..., None] * out["dir"]
        n_ref = (p - c) / np.linalg.norm(p - c, axis=-1, keepdims=True)
        ang = np.degrees(np.arccos(np.clip((out["normal"] * n_ref).sum(-1), -1.0, 1.0)))[inner]
        assert np.median(ang) <= 2.0, np.median(ang)
        shade_ref = synthetic.sh_basis(n_ref) @ synthetic.SH_TRUE
        assert np.median(np.abs(out["intensity"] - 0.7 * shade_ref)[inner]) <= 0.01
        assert np.all(out["depth"][~out["hit"]] == 0.0)
        # the rays go back through their pixels under the forward camera model (the undistortion inverts it)
        hv, hu = np.nonzero(out["hit"])
        pu, pv = render_twin.project(cam, cam["eye"] + out["depth"][hv, hu, None] * out["dir"][hv, hu])
        assert np.abs(pu - hu).max() < 1e-3 and np.abs(pv - hv).max() < 1e-3
