#!/usr/bin/env python3
"""Point-set registration (i3d_register_points) on bench.py's default workload (its build_workload: the 8 M-voxel sphere shell).

    python tools/register_bench.py [--points 1000000] [--rot-deg 0.1] [--trans-vox 1.0] [--depth-frames [--frames 40]]

Points leg: the ground-truth surface points of tools/query_bench.py (the zero set of the scene's sdf along seeded random directions) are moved by a seeded rigid
motion about the sphere's centre (--rot-deg, --trans-vox; the basin is the stored band of 3.5 voxels) and registered back from the identity, in brick-coherent
order and after a seeded shuffle.  Reports per order the host ms per call (one upload of the points, the whole budget launched back to back, two
synchronisations), iterations, status, the pose error against the inverse of the motion (degrees, voxels at the centre), and the mean |distance| of
i3d_query_points over the points before and after; and the coherent-to-shuffled ratio of the ms per call.
--depth-frames: the frames of tools/track_bench.py (the model ray-cast at the keyframe poses, starts perturbed by --frame-rot-deg / --frame-trans-vox) are
registered twice in the same session: by i3d_track_frame from the world -> camera start, and by i3d_register_points on the frame's back-projected camera-frame
points (the host back-projection is not timed) from the inverse, camera -> world start.  Reports ms per frame and the pose errors of both, side by side.
Prints one JSON line.
"""
import argparse, json, math, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "tests"))
from intrinsic3d_amd import binding, synthetic
import bench
import query_bench
import render_twin
import track_twin


def rigid_inverse(pose6):
    R = synthetic.aa_to_rotmat(np.asarray(pose6[:3], np.float64))
    return np.concatenate([synthetic.rotmat_to_aa(R.T), -R.T @ np.asarray(pose6[3:], np.float64)])


def apply(pose6, p):
    return p @ synthetic.aa_to_rotmat(np.asarray(pose6[:3], np.float64)).T + np.asarray(pose6[3:], np.float64)


def pose_error(a, b, centre, vs):
    """rotation between the two poses (degrees) and the distance between the images of `centre` (voxels)"""
    D = synthetic.aa_to_rotmat(np.asarray(a[:3], np.float64)) @ synthetic.aa_to_rotmat(np.asarray(b[:3], np.float64)).T
    ang = math.degrees(math.acos(min(1.0, max(-1.0, 0.5 * (np.trace(D) - 1.0)))))
    return ang, float(np.linalg.norm(apply(a, centre[None])[0] - apply(b, centre[None])[0])) / vs


def mean_abs_distance(ctx, pts, vs):
    st = ctx.query_points(pts, outputs=(), refined=False)["stats"]
    return st["sum_abs_distance"] / max(1, st["projected"]) / vs, st["projected"] / pts.shape[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000); ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--voxels", type=float, default=8.0e6); ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--voxel-size", type=float, default=0.001); ap.add_argument("--band", type=float, default=3.5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--rot-deg", type=float, default=0.1); ap.add_argument("--trans-vox", type=float, default=1.0)
    ap.add_argument("--depth-frames", action="store_true"); ap.add_argument("--frame-rot-deg", type=float, default=0.1); ap.add_argument("--frame-trans-vox", type=float, default=1.0)
    ap.add_argument("--iterations", type=int, default=None); ap.add_argument("--max-distance", type=float, default=None)
    a = ap.parse_args()
    log = lambda m: print(f"[register_bench] {m}", file=sys.stderr)
    if not a.depth_frames:
        a.frames = 1; a.width, a.height = 64, 48               # the grid alone: the keyframes are not read
    sc = bench.build_workload(a, log)
    g = bench.grid_arrays(sc); vs = float(np.float32(sc["voxel_size"]))
    centre = np.asarray(sc["scene"].c, np.float64)
    desc = {}
    if a.iterations is not None:
        desc["iterations"] = a.iterations
    if a.max_distance is not None:
        desc["max_distance"] = a.max_distance
    out = {"voxels": int(g["keys"].shape[0]), "points": a.points, "repeat": a.repeat}
    with binding.Context(0) as ctx:
        ctx.set_grid(vs, g["keys"], g["sdf"], g["sdf_refined"], g["albedo"], g["weight"], g["color"])
        rng = np.random.default_rng(a.seed)
        surf, _ = query_bench.surface_points(sc["scene"], a.points, rng, vs)
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
        dt = rng.normal(size=3); dt *= a.trans_vox * vs / np.linalg.norm(dt)
        Rm = synthetic.aa_to_rotmat(ax * math.radians(a.rot_deg))
        motion = np.concatenate([synthetic.rotmat_to_aa(Rm), centre - Rm @ centre + dt])      # about the centre
        moved = apply(motion, surf)
        truth = rigid_inverse(motion)
        orders = {"coherent": query_bench.brick_order(moved, vs), "shuffled": np.random.default_rng(7).permutation(moved.shape[0])}
        legs = {}
        for oname, idx in orders.items():
            p = np.ascontiguousarray(moved[idx])
            ctx.register_points(p, np.zeros(6), refined=False, **desc)                        # warm-up: the scratch grows
            t0 = time.time()
            for _ in range(a.repeat):
                pose, st = ctx.register_points(p, np.zeros(6), refined=False, **desc)
            t = (time.time() - t0) / a.repeat
            before, frac0 = mean_abs_distance(ctx, p, vs)
            after, frac1 = mean_abs_distance(ctx, apply(pose, p), vs)
            e_deg, e_vox = pose_error(pose, truth, centre, vs)
            legs[oname] = {"ms_per_call": 1e3 * t, "points_per_s_per_iteration": p.shape[0] * (st["iterations"] + 1) / t, "iterations": st["iterations"], "status": st["status"],
                           "valid": st["valid"], "inliers": st["inliers"], "rms_initial_vox": st["rms_initial"] / vs, "rms_final_vox": st["rms_final"] / vs,
                           "min_pivot_ratio": st["min_pivot_ratio"], "pose_error_deg": e_deg, "pose_error_vox": e_vox,
                           "mean_abs_distance_vox_before": before, "mean_abs_distance_vox_after": after, "projected_fraction_before": frac0, "projected_fraction_after": frac1}
        legs["coherent_to_shuffled_ms"] = legs["coherent"]["ms_per_call"] / legs["shuffled"]["ms_per_call"]
        out["points_leg"] = {"motion_deg": a.rot_deg, "motion_vox": a.trans_vox, **legs}
        if a.depth_frames:
            ctx.set_frames(sc["frames"], 1)
            ctx.set_camera(sc["intr"], sc["dist"], sc["poses"])
            intr, dist, poses = ctx.get_camera()
            nf = min(a.frames, len(poses))
            frng = np.random.default_rng(7)
            views = [ctx.render_view(frame=f, refined=False, planes=("depth",))["depth"] for f in range(nf)]
            starts = [track_twin.perturb(poses[f], frng, a.frame_rot_deg, a.frame_trans_vox * vs) for f in range(nf)]
            ident = dict(R=np.eye(3), eye=np.zeros(3), intr=np.asarray(intr, np.float64), dist=np.asarray(dist, np.float64), w=a.width, h=a.height)
            rays, _ = render_twin.rays(ident)
            pts = []
            for d in views:
                z = d.reshape(-1).astype(np.float64)
                pts.append(np.ascontiguousarray((rays * z[:, None])[z > 0]))
            c2w = [rigid_inverse(s) for s in starts]
            track = lambda f: ctx.track_frame(views[f], starts[f], refined=False)
            reg = lambda f: ctx.register_points(pts[f], c2w[f], refined=False, **desc)
            modes = [("track_frame", track), ("register_points", reg)]
            t_total = {m: 0.0 for m, _ in modes}; results = {}
            for m, fn in modes:
                fn(0)
            for r in range(a.repeat):                                                         # the two alternate: one session, one build
                for m, fn in modes:
                    t1 = time.time()
                    res = [fn(f) for f in range(nf)]
                    t_total[m] += time.time() - t1
                    if r == 0:
                        results[m] = res
            fr = {"frames": nf, "image": [a.width, a.height], "points_per_frame_mean": float(np.mean([p.shape[0] for p in pts])), "start_deg": a.frame_rot_deg,
                  "start_vox": a.frame_trans_vox}
            for m, _ in modes:
                w2c = [p if m == "track_frame" else rigid_inverse(p) for p, _ in results[m]]
                rot = np.array([track_twin.rot_err_deg(w2c[f], poses[f]) for f in range(nf)])
                cen = np.array([track_twin.centre_err(w2c[f], poses[f]) / vs for f in range(nf)])
                its = [s["iterations"][0] if m == "track_frame" else s["iterations"] for _, s in results[m]]
                status = [s["status"] for _, s in results[m]]
                fr[m] = {"host_ms_per_frame": 1e3 * t_total[m] / (nf * a.repeat), "mean_iterations": float(np.mean(its)),
                         "status_counts": {str(k): status.count(k) for k in sorted(set(status))}, "error_deg_median": float(np.median(rot)), "error_deg_max": float(rot.max()),
                         "error_vox_median": float(np.median(cen)), "error_vox_max": float(cen.max())}
            fr["track_to_register_ms"] = fr["track_frame"]["host_ms_per_frame"] / fr["register_points"]["host_ms_per_frame"]
            out["depth_frames_leg"] = fr
    print(json.dumps(out))


if __name__ == "__main__":
    main()
