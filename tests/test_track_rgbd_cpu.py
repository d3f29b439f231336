"""i3d_track_frame_rgbd without a device: the ctypes mirrors of its structs and its defaults, the derivatives of its numpy statement (track_rgbd_twin.py)
against central differences, and that statement on a smooth sphere, where depth cannot see a rotation about the centre and the model's intensity can.

The smooth scene, its starts and its descriptor are track_cases.py's, shared with test_gpu_track_rgbd.py: the device's bars of 0.02 degrees / 0.05 voxel hold provided this twin
ends within a fifth of them from the same starts, which test_colour_pins_what_depth_cannot_twin asserts.  Measured here (160 x 120, radius 16 voxels, the
scene's albedo, SH_TRUE, starts orbited by 2 degrees and moved by 3 voxels, w_g = 1, w_p = 0.1): 0.0004 / 0.0018 / 0.0010 degrees and 0.0002 / 0.0012 / 0.0006
voxel, status 0 after 35-39 iterations; depth only (w_p = 0): 4.0 / 10.0 / 5.1 degrees, status 1."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import render_twin
import track_rgbd_twin as rgbd_twin
import track_twin
from track_cases import BAR_DEG, BAR_VOX, DESC, DIST, WEIGHTS, smooth_scene, smooth_starts, voxel_sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def twin_model(sc):
    """model_fn of track_rgbd_twin.track_rgbd over render_twin's cast of the scene's voxels (true albedo, SH_TRUE)"""
    grid = render_twin.Grid(sc["keys"], sc["sdf"].astype(np.float64), sc["weight"], sc["voxel_size"], albedo=sc["albedo_true"], sh=voxel_sh(sc))

    def model(level, cam, ref):
        o = render_twin.render(grid, dict(R=ref["R"], eye=ref["eye"], intr=cam["intr"], dist=cam["dist"], w=cam["w"], h=cam["h"]))
        return o["depth"].astype(np.float32), o["normal"].astype(np.float32), o["intensity"].astype(np.float32)
    return model


def test_rgbd_struct_layouts_and_defaults():
    from intrinsic3d_amd import binding
    fields = {"i3d_track_rgbd_desc": binding.TrackRgbdDesc, "i3d_track_rgbd_stats": binding.TrackRgbdStats}
    body = "".join(f'printf("%zu\\n", sizeof({n}));' for n in fields)
    for n, cls in fields.items():
        body += "".join(f'printf("%zu\\n", offsetof({n}, {f}));' for f, _ in cls._fields_)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "intrinsic3d_hip.h"\nint main(){' + body + 'return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    want = [ctypes.sizeof(c) for c in fields.values()]
    for cls in fields.values():
        want += [getattr(cls, f).offset for f, _ in cls._fields_]
    assert got == want
    for name in ("i3d_track_rgbd_desc_default", "i3d_track_frame_rgbd", "i3d_debug_track_rgbd_sums"):
        assert name in binding.EXPORTS
    d = binding.track_rgbd_desc_default()
    b = binding.track_desc_default()
    assert bytes(d.base) == bytes(b)
    assert (d.geometric_weight, d.photo_weight, d.max_photo_residual, d.pad) == (1.0, 0.1, 0.0, 0)
    d = binding.track_rgbd_desc_default(photo_weight=0.25, levels=2, iterations=[7, 3])
    assert d.photo_weight == 0.25 and d.base.levels == 2 and list(d.base.iterations) == [7, 3, 0, 0] and d.base.use_refined_sdf == 1


def test_twin_derivatives_match_central_differences():
    sc = smooth_scene()
    vs = float(sc["voxel_size"])
    model = twin_model(sc)
    rng = np.random.default_rng(3)
    q = np.stack([rng.uniform(-0.15, 0.15, 500), rng.uniform(-0.1, 0.1, 500), rng.uniform(0.3, 0.6, 500)], -1)
    for dist in (np.zeros(5), DIST):
        cam = track_twin.level_camera(sc["intr"], dist, sc["width"], sc["height"], 0)
        assert rgbd_twin.check_projection_jacobian(cam, q) < 1e-8
        ref = track_twin.ref_from_pose(track_twin.perturb(sc["truth"], rng, 0.7, 1.5 * vs))
        Rc, tc = track_twin.pose_to_cw(track_twin.perturb(sc["truth"], rng, 0.5, 1.0 * vs))
        md, mn, mi = model(0, cam, ref)
        depth, _, lum = model(0, cam, track_twin.ref_from_pose(sc["truth"]))
        vtx, nrm = track_twin.frame_points(depth, cam)
        g = track_twin.associate(vtx, nrm, md, mn, cam, ref, Rc, tc, 0.05, 0.8)
        err, n = rgbd_twin.check_photo_rows(vtx, g["mask"], md, mi, lum, cam, ref, Rc, tc, 0.05)
        assert n > 3000 and err < 1e-6, (err, n)
        # the combined sums with w_g = 1 and no photometric term are track_twin's
        a = rgbd_twin.associate_rgbd(vtx, nrm, md, mn, mi, lum, cam, ref, Rc, tc, 0.05, 0.8, 1.0, 0.0)
        assert np.array_equal(a["sums"][:29], g["sums"]) and a["samples"] == 0
        a = rgbd_twin.associate_rgbd(vtx, nrm, md, mn, mi, lum, cam, ref, Rc, tc, 0.05, 0.8, 1.0, 0.1)
        assert 0.9 * g["inliers"] < a["samples"] <= g["inliers"] and a["sums"][29] > 0.0


def test_colour_pins_what_depth_cannot_twin():
    sc = smooth_scene()
    vs = float(sc["voxel_size"])
    model = twin_model(sc)
    dist = np.zeros(5)
    cam0 = track_twin.level_camera(sc["intr"], dist, sc["width"], sc["height"], 0)
    depth, _, lum = model(0, cam0, track_twin.ref_from_pose(sc["truth"]))
    assert (depth > 0).sum() > 0.2 * depth.size
    desc = track_twin.default_desc(**dict(DESC, iterations=DESC["iterations"] + [0, 0, 0]))
    for start in smooth_starts(sc):
        r0 = track_twin.rot_err_deg(start, sc["truth"])
        assert r0 > 1.9
        pose_d, st_d = rgbd_twin.track_rgbd(depth, lum, sc["intr"], dist, start, model, desc, 1.0, 0.0)
        pose_c, st_c = rgbd_twin.track_rgbd(depth, lum, sc["intr"], dist, start, model, desc, WEIGHTS["geometric_weight"], WEIGHTS["photo_weight"])
        rd = track_twin.rot_err_deg(pose_d, sc["truth"])
        rc, cc = track_twin.rot_err_deg(pose_c, sc["truth"]), track_twin.centre_err(pose_c, sc["truth"]) / vs
        print(f"start {r0:.3f} deg: depth only {rd:.4f} deg (status {st_d['status']}); rgbd {rc:.5f} deg {cc:.5f} voxel (status {st_c['status']}, "
              f"{st_c['iterations'][0]} iterations), min_pivot_ratio {st_d['min_pivot_ratio']:.2e} -> {st_c['min_pivot_ratio']:.2e}")
        assert rd >= 0.9 * r0, (rd, r0)                                   # depth alone leaves the rotation error where it was, or worse
        assert st_c["status"] == 0 and rc < BAR_DEG / 5 and cc < BAR_VOX / 5, (rc, cc, st_c)
        assert st_c["min_pivot_ratio"] > st_d["min_pivot_ratio"] and st_c["photo_samples"] > 0.9 * st_c["inliers"]
        assert st_c["photo_rms_final"] < 0.05 * st_c["photo_rms_initial"]
