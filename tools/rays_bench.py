#!/usr/bin/env python3
"""Throughput of i3d_cast_rays on bench.py's default workload (its build_workload: the 8 M-voxel sphere shell, keyframes of 640x480, noisy poses): the camera
rays of one keyframe (a) in row-major pixel order and (b) under a seeded shuffle, each with order = 0 and order = 1, and i3d_render_view of the same camera
beside them, alternated in one session.

    python tools/rays_bench.py [--voxels 8e6] [--frames 8] [--frame 0] [--repeat 5] [--supersample 1] [--color [--fusion-frames 8]]

--color: Context.cast_rays_color on both ray sets with order 0 and 1 ("color_*", beside the t-only "cast_*_t" of the same rays),
Context.render_view_color of the same camera, and on a volume fused from the first --fusion-frames keyframes Fusion.cast_rays_color beside the t-only
Fusion.cast_rays, all in the same alternation.

Prints one JSON line: per variant the host ms per call (the call as a caller sees it: uploads, launches, one synchronisation, the copies back), the spread
over the repeats, rays/s and samples per ray; with all outputs and with t alone.  The kernels' own times come from a kernel trace of this command
(rocprofv3 --kernel-trace --stats -- python tools/rays_bench.py ...), in a run of its own.
"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from intrinsic3d_amd import binding, synthetic
import bench


def camera_rays(pose6, intr, dist, w, h, ss=1):
    """eye and the directions R^T (x, y, 1) of the integer pixels, row-major, (x, y) undistorted by the fixed-point iteration of the renderer; ss > 1: ss x ss rays
    per pixel, at the pixel coordinates (u + i / ss, v + j / ss)"""
    R = synthetic.aa_to_rotmat(np.asarray(pose6[:3], np.float64)); t = np.asarray(pose6[3:], np.float64)
    fx, fy, cx, cy = intr
    v, u = np.meshgrid(np.arange(h * ss, dtype=np.float64) / ss, np.arange(w * ss, dtype=np.float64) / ss, indexing="ij")
    xd = ((u - cx) / fx).ravel(); yd = ((v - cy) / fy).ravel()
    x, y = xd.copy(), yd.copy()
    k1, k2, k3, p1, p2 = dist
    if not (np.abs(dist) <= 1e-5).all():
        for _ in range(10):
            r2 = x * x + y * y; r4 = r2 * r2; r6 = r4 * r2
            dc = 1.0 + k1 * r2 + k2 * r4 + k3 * r6
            x, y = (xd - (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) / dc, (yd - (2.0 * p2 * xd * y + p1 * (r2 + 2.0 * y * y))) / dc
    d = np.stack([(R[0, a] * x + R[1, a] * y) + R[2, a] for a in range(3)], -1)
    eye = -(R.T @ t)
    return np.broadcast_to(eye, d.shape).copy(), np.ascontiguousarray(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=float, default=8.0e6); ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--voxel-size", type=float, default=0.001); ap.add_argument("--band", type=float, default=3.5)
    ap.add_argument("--seed", type=int, default=1234); ap.add_argument("--repeat", type=int, default=5); ap.add_argument("--frame", type=int, default=0)
    ap.add_argument("--supersample", type=int, default=1, help="rays per pixel edge of the cast variants (render_view stays at one ray per pixel)")
    ap.add_argument("--color", action="store_true", help="also time cast_rays_color beside the t-only cast_rays of the same rays, in the same alternation")
    ap.add_argument("--fusion-frames", type=int, default=8, help="--color: keyframes fused into the volume of the fusion figures (0: no volume)")
    a = ap.parse_args()
    sc = bench.build_workload(a, lambda m: print(f"[rays_bench] {m}", file=sys.stderr))
    g = bench.grid_arrays(sc)
    n = g["keys"].shape[0]; vs = float(sc["voxel_size"])
    with binding.Context(0) as ctx:
        ctx.set_grid(vs, g["keys"], g["sdf"], g["sdf_refined"], g["albedo"], g["weight"], g["color"])
        ctx.set_frames(sc["frames"], 1)
        ctx.set_camera(sc["intr"], sc["dist"], sc["poses"])
        ctx.set_voxel_sh(np.tile(synthetic.SH_TRUE, (n, 1)))
        intr, dist, poses = ctx.get_camera()
        o, d = camera_rays(poses[a.frame], intr, dist, a.width, a.height, a.supersample)
        perm = np.random.default_rng(a.seed).permutation(o.shape[0])
        sets = {"rows": (o, d), "shuffled": (np.ascontiguousarray(o[perm]), np.ascontiguousarray(d[perm]))}
        planes = ("depth", "normal", "albedo", "shading", "intensity")
        variants = {"render_view_planes": lambda: ctx.render_view(frame=a.frame, planes=planes), "render_view_depth": lambda: ctx.render_view(frame=a.frame, planes=("depth",))}
        for name, (ro, rd) in sets.items():
            for order in (0, 1):
                variants[f"cast_{name}_order{order}_all"] = lambda ro=ro, rd=rd, order=order: ctx.cast_rays(ro, rd, outputs=binding.CAST_OUTPUTS, order=order)
                variants[f"cast_{name}_order{order}_t"] = lambda ro=ro, rd=rd, order=order: ctx.cast_rays(ro, rd, outputs=("t",), order=order)
        vol = None
        if a.color:                                          # the colour call beside the t-only call of the same rays, alternated with the rest
            for name, (ro, rd) in sets.items():
                for order in (0, 1):
                    variants[f"color_{name}_order{order}"] = lambda ro=ro, rd=rd, order=order: ctx.cast_rays_color(ro, rd, order=order)
            variants["render_view_color"] = lambda: ctx.render_view_color(frame=a.frame)
            if a.fusion_frames > 0:                          # the same pair on a volume fused from the first keyframes
                from render_bench import fused_volume
                vol = fused_volume(sc, a.fusion_frames)
                ro, rd = sets["rows"]
                variants["fusion_cast_rows_order0_t"] = lambda: vol.cast_rays(ro, rd, outputs=("t",))
                variants["fusion_color_rows_order0"] = lambda: vol.cast_rays_color(ro, rd)
        stats = {}
        for k, fn in variants.items():                       # warm-up: the bitmap, every scratch at its final size
            stats[k] = fn()["stats"]
        times = {k: [] for k in variants}
        for _ in range(a.repeat):                            # alternated: every variant once per round
            for k, fn in variants.items():
                t1 = time.perf_counter(); fn(); times[k].append(1e3 * (time.perf_counter() - t1))
        if vol is not None:
            vol.close()
    res = {}
    for k in variants:
        ms = float(np.median(times[k]))
        rays = a.width * a.height * (a.supersample ** 2 if not k.startswith("render_view") else 1)
        res[k] = {"ms_median": ms, "ms_min": float(min(times[k])), "ms_max": float(max(times[k])), "rays_per_s": rays / (1e-3 * ms),
                  "rays": rays, "samples_per_ray": stats[k]["samples"] / rays, "hits": stats[k]["hits"]}
    print(json.dumps({"voxels": n, "image": [a.width, a.height], "frame": a.frame, "supersample": a.supersample, "repeat": a.repeat, "variants": res}))


if __name__ == "__main__":
    main()
