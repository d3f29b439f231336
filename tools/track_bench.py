#!/usr/bin/env python3
"""Frame registration (i3d_track_frame) on bench.py's default workload (its build_workload: the 8 M-voxel sphere shell, keyframes of 640x480).  Each frame is the
model ray-cast (i3d_render_view, fused SDF) at a keyframe's pose, which is the truth here; tracking starts from that pose perturbed by --rot-deg about a random
axis and --trans-vox voxels in a random direction.

    python tools/track_bench.py [--voxels 8e6] [--frames 40] [--repeat 2] [--rgbd [--photo-weight 0.1]] [--sdf [--stride 1] [--huber-vox 0] [--batch B[,B...]]]

--rgbd registers by depth and model intensity (i3d_track_frame_rgbd): every voxel gets the scene's SH, a frame's luminance is the model's intensity cast at the
true pose, and the line carries the depth-only figures of the same frames, timed in alternation, under "depth_only".

--sdf registers the same frames from the same starts on the stored field, without a ray cast (i3d_track_frame_sdf), timed in alternation
with the ICP registration, whose figures the line carries under "depth_only".  The basin of the direct registration is the stored band (--band): a start
further off than that (--trans-vox) leaves it.

--sdf --batch B registers the first B frames from the same starts as one batch (i3d_track_frames_sdf) and as B single calls, timed in
alternation in the same session, and prints one JSON line per B: ms per frame of both (every timed round, their median and range), the largest difference
between the two sets of returned poses - which must be 0 - and whether every field of the stats agrees.  B may be a comma-separated list (one workload, one
session); the workload gets max(B) keyframes.  The ICP registration is not timed in this mode.

--sdf --rgbd registers on the stored field with the photometric term (i3d_track_frame_sdf_rgbd) and times it in alternation with
i3d_track_frame_sdf and i3d_track_frame_rgbd on the same frames from the same starts (the ICP registration is not timed in this mode); the line carries those
two under "sdf" and "rgbd".  With --batch B the batch form (i3d_track_frames_sdf_rgbd) is timed against B single calls as above.

Prints one JSON line: host ms per frame (the call as a caller sees it: the upload, every pass's launches and synchronisation, the final figures), frame pixels
per second, mean iterations per level, status counts, pose error after tracking (median / max, degrees and voxels), RMS before / after.  The kernels' own times
come from a kernel trace of this command (rocprofv3 --kernel-trace --stats).
"""
import argparse, json, math, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from intrinsic3d_amd import binding
import bench
import track_twin


def batch_lines(a, ctx, views, starts, poses, sdesc, single, sizes, vs, n):
    """one JSON line per batch size: the first B frames as one i3d_track_frames_sdf call and as B i3d_track_frame_sdf calls, timed in alternation (with --rgbd:
    i3d_track_frames_sdf_rgbd and i3d_track_frame_sdf_rgbd)"""
    for B in sizes:
        if B > len(views):
            raise SystemExit(f"--batch {B}: the workload has {len(views)} frames")
        depths = np.stack([views[f]["depth"] for f in range(B)]).astype(np.float32); st0 = np.stack(starts[:B])
        if a.rgbd:
            lums = np.stack([views[f]["intensity"] for f in range(B)]).astype(np.float32)
            batch = lambda: ctx.track_frames_sdf_rgbd(depths, lums, st0, refined=False, use_context_camera=1, photo_weight=a.photo_weight, **sdesc)
        else:
            batch = lambda: ctx.track_frames_sdf(depths, st0, refined=False, use_context_camera=1, **sdesc)
        loop = lambda: [single(f) for f in range(B)]
        batch(); loop()                                # warm-up: buffers grown
        rounds = max(a.repeat, min(50, 200 // B))      # a round of a small batch is short: about 200 registrations per figure
        tb, ts = [], []
        for _ in range(rounds):
            t1 = time.time(); got = batch(); tb.append(1e3 * (time.time() - t1) / B)
            t1 = time.time(); ref = loop(); ts.append(1e3 * (time.time() - t1) / B)
        diff = max(float(np.abs(got[0][f] - ref[f][0]).max()) for f in range(B))
        same_bits = all(got[0][f].tobytes() == np.asarray(ref[f][0]).tobytes() and got[1][f] == ref[f][1] for f in range(B))
        rot = np.array([track_twin.rot_err_deg(got[0][f], poses[f]) for f in range(B)])
        cen = np.array([track_twin.centre_err(got[0][f], poses[f]) / vs for f in range(B)])
        status = [s["status"] for s in got[1]]
        fig = lambda t: {"ms_per_frame_median": float(np.median(t)), "ms_per_frame_min": float(np.min(t)), "ms_per_frame_max": float(np.max(t)),
                         "ms_per_frame_rounds": [round(x, 4) for x in t]}
        print(json.dumps({"batch": B, "entry_point": "i3d_track_frames_sdf_rgbd" if a.rgbd else "i3d_track_frames_sdf", "voxels": n, "image": [a.width, a.height], "stride": a.stride, "huber_vox": a.huber_vox, "rounds": rounds,
                          "batched": fig(tb), "single_calls": fig(ts), "speedup_median": float(np.median(ts) / np.median(tb)),
                          "max_pose_difference": diff, "poses_and_stats_bit_identical": bool(same_bits),
                          "mean_iterations": float(np.mean([s["iterations"] for s in got[1]])), "max_iterations": int(max(s["iterations"] for s in got[1])),
                          "status_counts": {str(k): status.count(k) for k in sorted(set(status))},
                          "error_deg_median": float(np.median(rot)), "error_vox_median": float(np.median(cen))}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxels", type=float, default=8.0e6); ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--voxel-size", type=float, default=0.001); ap.add_argument("--band", type=float, default=3.5)
    ap.add_argument("--seed", type=int, default=1234); ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--rot-deg", type=float, default=1.0); ap.add_argument("--trans-vox", type=float, default=3.0)
    ap.add_argument("--rgbd", action="store_true", help="register with i3d_track_frame_rgbd; the depth-only registration of the same frames is timed alongside")
    ap.add_argument("--photo-weight", type=float, default=0.1)
    ap.add_argument("--sdf", action="store_true", help="register with i3d_track_frame_sdf; the ICP registration of the same frames is timed alongside")
    ap.add_argument("--stride", type=int, default=1); ap.add_argument("--huber-vox", type=float, default=0.0, help="huber_delta in voxels (0: off)")
    ap.add_argument("--iterations", type=int, default=None, help="level-0 budget (default: the library's)")
    ap.add_argument("--stop", type=float, default=None, help="stop_rotation = stop_translation (default: the library's)")
    ap.add_argument("--batch", type=str, default=None, help="with --sdf: batch sizes B[,B...]; i3d_track_frames_sdf on the first B frames against B single calls")
    a = ap.parse_args()
    sizes = sorted({int(x) for x in a.batch.split(",")}) if a.batch else []
    if sizes:
        if not a.sdf or sizes[0] < 1:
            ap.error("--batch needs --sdf and sizes >= 1")
        a.frames = sizes[-1]
    sc = bench.build_workload(a, lambda m: print(f"[track_bench] {m}", file=sys.stderr))
    g = bench.grid_arrays(sc)
    n = g["keys"].shape[0]; vs = float(sc["voxel_size"])
    nf = min(a.frames, len(sc["poses"]))
    rng = np.random.default_rng(7)
    desc = {}
    if a.iterations is not None:
        desc["iterations"] = [a.iterations]
    if a.stop is not None:
        desc.update(stop_rotation=a.stop, stop_translation=a.stop)
    with binding.Context(0) as ctx:
        ctx.set_grid(vs, g["keys"], g["sdf"], g["sdf_refined"], g["albedo"], g["weight"], g["color"])
        ctx.set_frames(sc["frames"], 1)
        ctx.set_camera(sc["intr"], sc["dist"], sc["poses"])
        intr, dist, poses = ctx.get_camera()
        if a.rgbd:                                     # the frame's luminance is what the model predicts at the true pose: albedo x the scene's SH at every voxel
            from intrinsic3d_amd import synthetic
            ctx.set_voxel_sh(np.tile(synthetic.SH_TRUE, (n, 1)))
        views = [ctx.render_view(frame=f, refined=False, planes=("depth", "intensity") if a.rgbd else ("depth",)) for f in range(nf)]
        starts = [track_twin.perturb(poses[f], rng, a.rot_deg, a.trans_vox * vs) for f in range(nf)]
        depth_only = lambda f: ctx.track_frame(views[f]["depth"], starts[f], refined=False, **desc)
        rgbd = lambda f: ctx.track_frame_rgbd(views[f]["depth"], views[f]["intensity"], starts[f], refined=False, photo_weight=a.photo_weight, **desc)
        sdesc = dict(stride=a.stride, huber_delta=a.huber_vox * vs)
        if a.iterations is not None:
            sdesc["iterations"] = a.iterations
        if a.stop is not None:
            sdesc.update(stop_rotation=a.stop, stop_translation=a.stop)
        sdf = lambda f: ctx.track_frame_sdf(views[f]["depth"], starts[f], refined=False, use_context_camera=1, **sdesc)
        sdf_rgbd = lambda f: ctx.track_frame_sdf_rgbd(views[f]["depth"], views[f]["intensity"], starts[f], refined=False, use_context_camera=1,
                                                      photo_weight=a.photo_weight, **sdesc)
        if sizes:
            batch_lines(a, ctx, views, starts, poses, sdesc, sdf_rgbd if a.rgbd else sdf, sizes, vs, n)
            return
        if a.sdf and a.rgbd:                           # the three trackers that see the same frame, in one session
            modes = [("sdf_rgbd", sdf_rgbd), ("sdf", sdf), ("rgbd", rgbd)]
        else:
            modes = [("depth_only", depth_only)] + ([("rgbd", rgbd)] if a.rgbd else []) + ([("sdf", sdf)] if a.sdf else [])
        t_total = {m: 0.0 for m, _ in modes}; results = {}
        for m, fn in modes:
            fn(0)                                      # warm-up: buffers grown
        for r in range(a.repeat):                      # with --rgbd the two registrations alternate: one session, one build
            for m, fn in modes:
                t1 = time.time()
                out = [fn(f) for f in range(nf)]
                t_total[m] += time.time() - t1
                if r == 0:
                    results[m] = out
    calls = nf * a.repeat
    rot0 = np.array([track_twin.rot_err_deg(starts[f], poses[f]) for f in range(nf)])

    def figures(m):
        res = results[m]
        rot = np.array([track_twin.rot_err_deg(p, poses[f]) for f, (p, _) in enumerate(res)])
        cen = np.array([track_twin.centre_err(p, poses[f]) / vs for f, (p, _) in enumerate(res)])
        its = np.array([s["iterations"] for _, s in res], np.float64).reshape(len(res), -1)
        status = [s["status"] for _, s in res]
        out = {"voxels": n, "frames": nf, "image": [a.width, a.height], "calls_timed": calls, "host_ms_per_frame": 1e3 * t_total[m] / calls,
               "frame_pixels_per_s": a.width * a.height * calls / t_total[m], "levels": 1, "mean_iterations_per_level": its.mean(0).tolist(),
               "status_counts": {str(k): status.count(k) for k in sorted(set(status))},
               "start_error_deg_median": float(np.median(rot0)), "start_error_vox": a.trans_vox,
               "error_deg_median": float(np.median(rot)), "error_deg_max": float(rot.max()), "error_vox_median": float(np.median(cen)), "error_vox_max": float(cen.max()),
               "rms_initial_mean_m": float(np.mean([s["rms_initial"] for _, s in res])), "rms_final_mean_m": float(np.mean([s["rms_final"] for _, s in res])),
               "min_pivot_ratio_median": float(np.median([s["min_pivot_ratio"] for _, s in res]))}
        if m in ("rgbd", "sdf_rgbd"):
            out.update(photo_weight=a.photo_weight, photo_samples_mean=float(np.mean([s["photo_samples"] for _, s in res])),
                       photo_rms_initial_mean=float(np.mean([s["photo_rms_initial"] for _, s in res])), photo_rms_final_mean=float(np.mean([s["photo_rms_final"] for _, s in res])))
        if m in ("sdf", "sdf_rgbd"):
            out.update(stride=a.stride, huber_vox=a.huber_vox, usable_pixels_mean=float(np.mean([s["valid_pixels"] for _, s in res])),
                       valid_mean=float(np.mean([s["valid"] for _, s in res])), inliers_mean=float(np.mean([s["inliers"] for _, s in res])))
        return out

    if a.sdf and a.rgbd:
        print(json.dumps(dict(figures("sdf_rgbd"), sdf=figures("sdf"), rgbd=figures("rgbd"))))
        return
    icp = figures("depth_only")
    out = icp
    if a.rgbd:
        out = dict(figures("rgbd"), depth_only=icp)
    if a.sdf:
        out = dict(figures("sdf"), depth_only=icp, **({"rgbd": out} if a.rgbd else {}))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
