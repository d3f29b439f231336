"""i3d_track_frame without a device: the ctypes mirrors of its structs, and the numpy statement of the registration (track_twin.py) on an analytic bumpy
sphere whose model planes are ray-cast analytically."""
import math
import os
import subprocess
import tempfile

import numpy as np

import track_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_track_struct_layouts_match_header():
    import ctypes
    from intrinsic3d_amd import binding
    fields = {"i3d_track_desc": binding.TrackDesc, "i3d_track_stats": binding.TrackStats}
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
    for name in ("i3d_track_desc_default", "i3d_track_frame", "i3d_debug_track_sums"):
        assert name in binding.EXPORTS


def test_twin_converges_on_analytic_bumpy_sphere():
    from intrinsic3d_amd import synthetic
    vs = 0.004
    scene = synthetic.Scene(np.array([0.11, 0.09, 0.12]), 16 * vs, 3.0 * vs, 60.0)      # bumps that pin rotation about the centre
    w, h = 160, 120
    fx = 525.0 * w / 640.0
    intr = np.array([fx, fx, (w - 1) * 0.5, (h - 1) * 0.5])
    dist = np.zeros(5)
    eye = scene.c + 3.2 * scene.R * np.array([0.3, 0.4, -0.87]) / np.linalg.norm([0.3, 0.4, -0.87])
    truth = synthetic.look_at_pose(eye, scene.c)
    cam0 = track_twin.level_camera(intr, dist, w, h, 0)
    depth, _ = track_twin.raycast_scene(scene, cam0, track_twin.ref_from_pose(truth))
    assert (depth > 0).sum() > 0.3 * w * h

    def model(level, cam, ref):
        return track_twin.raycast_scene(scene, cam, ref)

    desc = track_twin.default_desc(levels=2)
    rng = np.random.default_rng(4)
    for _ in range(2):
        start = track_twin.perturb(truth, rng, 2.0, 3 * vs)
        assert track_twin.rot_err_deg(start, truth) > 1.9
        pose, st = track_twin.track(depth, intr, dist, start, model, desc)
        assert st["status"] == 0, st
        assert track_twin.rot_err_deg(pose, truth) < 0.02 and track_twin.centre_err(pose, truth) < 0.05 * vs, (track_twin.rot_err_deg(pose, truth), track_twin.centre_err(pose, truth) / vs, st)
        assert st["min_pivot_ratio"] > 1e-9 and st["rms_final"] < 0.01 * vs and st["rms_initial"] > st["rms_final"]
    # at the truth the registration stays there
    pose, st = track_twin.track(depth, intr, dist, truth, model, desc)
    assert st["status"] == 0 and track_twin.centre_err(pose, truth) < 1e-3 * vs and track_twin.rot_err_deg(pose, truth) < 1e-3
    # an empty frame: too few inliers, the pose is returned as it came
    pose, st = track_twin.track(np.zeros_like(depth), intr, dist, truth, model, desc)
    assert st["status"] == 2 and np.array_equal(pose, truth)
