#!/usr/bin/env python3
"""Throughput of i3d_render_view on bench.py's default workload (its build_workload: the 8 M-voxel sphere shell, 200 keyframes of 640x480, noisy poses and
luminance): every keyframe at level 0, all planes, with the fused SDF, albedo 0.6 and the true SH.

    python tools/render_bench.py [--voxels 8e6] [--frames 200] [--repeat 2] [--color [--fusion-frames 8]]

--color: after the figures above, per keyframe the colour view (Context.render_view_color: colour and depth) in alternation with the
depth-only render_view of the same camera, --repeat rounds each, and the same pair on a volume fused from the first --fusion-frames keyframes
(Fusion.render_color against Fusion.render, depth only); host ms per call under "color".  The kernels' microseconds (k_render<G, true> beside k_render<G>)
come from a kernel trace of this command, like every kernel time here.

Prints one JSON line: host ms per view (the call as a caller sees it: launch, one synchronisation, the copies of all six planes), host ms per view of a stats-only
call (launch + synchronisation, no plane copied: the kernel's time plus the call overhead), rays/s, mean samples per ray, hit fraction, RMS residual over the
hits.  The kernel's own time comes from a kernel trace of this command (rocprofv3 --kernel-trace --stats).
"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from intrinsic3d_amd import binding, synthetic
import bench


def alternate(calls, rounds):
    """{name: fn} timed in alternation, every fn once per round after one warm-up each -> {name: [ms per call]}"""
    for fn in calls.values():
        fn()
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            t1 = time.perf_counter(); fn(); times[k].append(1e3 * (time.perf_counter() - t1))
    return times


def fused_volume(sc, frames):
    """the first `frames` keyframes of the workload fused into a volume (depth and colour, their own poses): the fusion model of the colour figures"""
    from make_dataset import pose_vec_to_cam_to_world
    f = binding.Fusion(sc["voxel_size"], 0.1, 10.0, initial_capacity=1 << 25)
    intr = np.asarray(sc["intr"], np.float32)
    for fr, p in list(zip(sc["frames"], sc["poses"]))[:frames]:
        f.integrate(fr["depth"][0], intr, fr["bgr"][0], intr, pose_vec_to_cam_to_world(np.asarray(p, np.float64)).astype(np.float32), 2)
    return f


def color_figures(a, ctx, sc):
    """--color: per keyframe the colour view and the depth-only view of the same camera in alternation, on the context and on a volume fused from the first
    --fusion-frames keyframes (seen through those keyframes' cameras) -> ms per call of each: median over all calls, and the spread of the per-view medians"""
    intr, dist, poses = ctx.get_camera()
    t = {}

    def add(times):
        for k, v in times.items():
            t.setdefault(k, []).append(v)
    for f in range(a.frames):
        add(alternate({"context_depth": lambda: ctx.render_view(frame=f, refined=False, planes=("depth",)),
                       "context_color": lambda: ctx.render_view_color(frame=f, refined=False)}, a.repeat))
    if a.fusion_frames > 0:
        with fused_volume(sc, a.fusion_frames) as vol:
            for f in range(min(a.frames, a.fusion_frames)):
                cam = dict(width=a.width, height=a.height, intr=intr, dist=dist, pose=poses[f])
                add(alternate({"fusion_depth": lambda: vol.render(cam, planes=("depth",)), "fusion_color": lambda: vol.render_color(cam)}, a.repeat))
    out = {"rounds_per_view": a.repeat, "fusion_frames": a.fusion_frames}
    for k, per_view in t.items():
        med = [float(np.median(v)) for v in per_view]
        out[k] = {"views": len(per_view), "ms_per_call_median": float(np.median(np.concatenate(per_view))), "view_median_min": min(med), "view_median_max": max(med)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=float, default=8.0e6); ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--voxel-size", type=float, default=0.001); ap.add_argument("--band", type=float, default=3.5)
    ap.add_argument("--seed", type=int, default=1234); ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--color", action="store_true", help="also time the colour view against the depth-only view of the same camera, in alternation")
    ap.add_argument("--fusion-frames", type=int, default=8, help="--color: keyframes fused into the volume of the fusion figures (0: no volume)")
    a = ap.parse_args()
    sc = bench.build_workload(a, lambda m: print(f"[render_bench] {m}", file=sys.stderr))
    g = bench.grid_arrays(sc)
    n = g["keys"].shape[0]; vs = float(sc["voxel_size"])
    with binding.Context(0) as ctx:
        ctx.set_grid(vs, g["keys"], g["sdf"], g["sdf_refined"], g["albedo"], g["weight"], g["color"])
        ctx.set_frames(sc["frames"], 1)
        ctx.set_camera(sc["intr"], sc["dist"], sc["poses"])
        ctx.set_voxel_sh(np.tile(synthetic.SH_TRUE, (n, 1)))
        t1 = time.time(); ctx.render_view(frame=0, planes=()); t_bricks = time.time() - t1      # first call: the brick bitmap is built
        ctx.render_view(frame=0)                                                                # warm-up of the planes' scratch
        hits = samples = 0; rsq = 0.0; t_full = 0.0; t_stats = 0.0
        for r in range(a.repeat):
            t1 = time.time()
            for f in range(a.frames):
                s = ctx.render_view(frame=f)["stats"]
                if r == 0:
                    hits += s["hits"]; samples += s["samples"]; rsq += s["residual_sq_sum"]
            t_full += time.time() - t1
            t1 = time.time()
            for f in range(a.frames):
                ctx.render_view(frame=f, planes=())
            t_stats += time.time() - t1
        colour = color_figures(a, ctx, sc) if a.color else None
    views = a.frames * a.repeat; rays = a.frames * a.width * a.height
    out = {"voxels": n, "frames": a.frames, "image": [a.width, a.height], "views_timed": views, "brick_build_first_call_ms": 1e3 * t_bricks,
           "host_ms_per_view_all_planes": 1e3 * t_full / views, "host_ms_per_view_stats_only": 1e3 * t_stats / views,
           "rays_per_s_all_planes": a.width * a.height * views / t_full, "mean_samples_per_ray": samples / rays, "hit_fraction": hits / rays,
           "rms_residual_over_hits": float(np.sqrt(rsq / max(1, hits)))}
    if colour is not None:
        out["color"] = colour
    print(json.dumps(out))


if __name__ == "__main__":
    main()
