#!/usr/bin/env python3
"""Throughput and surface-distance figures of i3d_query_points / i3d_fusion_query_points.

    python tools/query_bench.py [--points 1000000] [--voxels 8e6] [--refine-steps 0] [--fusion-frames 12] [--fusion-radius 150]

Context leg: the grid of bench.py's default workload (its build_workload: the 8 M-voxel sphere shell), queried for the fused field (sdf) and for the refined one
(sdf_refined).  The workload loads sdf_refined = sdf, so the two sets of figures coincide unless --refine-steps K > 0 is given: then the keyframes are set and K
Gauss-Newton iterations run first, and the refined figures are those of the optimised model.  Fusion leg: fusion_bench.py's sphere fused from --fusion-frames frames.
Points: N points of the analytic ground-truth surface (the zero set of the scene's sdf along seeded random directions; the visible side for the fusion leg), and
the same points displaced by up to +-1.5 voxels along the true normal.  Each set is queried in brick-coherent order (sorted by the key of the 8^3 brick on the host)
and after a seeded shuffle.  Prints one JSON line: per leg, field and order the host ms per call (upload, two launches, all arrays copied back, one
synchronisation), points/s, mean / RMS / max |distance| over the projected points, the projected fraction and Newton steps per valid point; the stats-only call
(nothing copied back) beside it; and the coherent-to-shuffled ratio of the points/s, of the full call and of the stats-only call.
"""
import argparse, json, math, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
from intrinsic3d_amd import binding, synthetic
import bench


def surface_points(scene, n, rng, vs, towards=None, min_dot=0.6):
    """n points with scene.sdf = 0 along random directions from the centre (safeguarded Newton on the radius), their true normals, and the displaced copies"""
    d = rng.normal(size=((8 if towards is not None else 1) * n, 3)); d /= np.sqrt((d * d).sum(1, keepdims=True))
    if towards is not None:
        d = d[d @ towards > min_dot]
    d = d[:n]
    r = np.full(d.shape[0], scene.R)
    for _ in range(30):
        r = r - scene.sdf(scene.c + d * r[:, None])           # d sdf / d r = 1 + O(amp * freq)
    p = scene.c + d * r[:, None]
    assert np.abs(scene.sdf(p)).max() < 1e-9 * vs
    return p, p + scene.normal(p) * (rng.uniform(-1.5, 1.5, p.shape[0]) * vs)[:, None]


def brick_order(p, vs):
    b = np.floor(p / vs).astype(np.int64) >> 3
    return np.lexsort((b[:, 0], b[:, 1], b[:, 2]))


def timed(query, pts, repeat, **kw):
    query(pts, **kw)                                           # warm-up: the scratch grows
    t0 = time.time()
    for _ in range(repeat):
        out = query(pts, **kw)
    return (time.time() - t0) / repeat, out["stats"]


def leg(query, sets, vs, repeat, fields):
    res = {}
    for fname, kw in fields.items():
        for sname, pts in sets.items():
            orders = {"coherent": pts[brick_order(pts, vs)], "shuffled": pts[np.random.default_rng(7).permutation(pts.shape[0])]}
            row = {}
            for oname, p in orders.items():
                t, st = timed(query, p, repeat, **kw)
                ts, _ = timed(query, p, repeat, outputs=(), **kw)
                n = p.shape[0]; m = max(1, st["projected"])
                row[oname] = {"ms_per_call": 1e3 * t, "points_per_s": n / t, "ms_per_call_stats_only": 1e3 * ts, "points_per_s_stats_only": n / ts,
                              "projected_fraction": st["projected"] / n, "valid_fraction": st["valid"] / n, "steps_per_valid_point": st["steps"] / max(1, st["valid"]),
                              "mean_abs_distance_vox": st["sum_abs_distance"] / m / vs, "rms_distance_vox": math.sqrt(st["sum_sq_distance"] / m) / vs,
                              "max_abs_distance_vox": st["max_abs_distance"] / vs}
            row["coherent_to_shuffled_full_call"] = row["coherent"]["points_per_s"] / row["shuffled"]["points_per_s"]
            row["coherent_to_shuffled_stats_only"] = row["coherent"]["points_per_s_stats_only"] / row["shuffled"]["points_per_s_stats_only"]
            res[f"{fname}/{sname}"] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000000); ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--voxels", type=float, default=8.0e6); ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--voxel-size", type=float, default=0.001); ap.add_argument("--band", type=float, default=3.5)
    ap.add_argument("--seed", type=int, default=1234); ap.add_argument("--refine-steps", type=int, default=0)
    ap.add_argument("--subvolume", type=float, default=0.06); ap.add_argument("--shell", type=float, default=1.0)
    ap.add_argument("--fusion-frames", type=int, default=12); ap.add_argument("--fusion-radius", type=int, default=150)
    ap.add_argument("--skip-context", action="store_true"); ap.add_argument("--skip-fusion", action="store_true")
    a = ap.parse_args()
    log = lambda m: print(f"[query_bench] {m}", file=sys.stderr)
    out = {"points": a.points, "repeat": a.repeat}
    if not a.skip_context:
        if a.refine_steps <= 0:
            a.frames = 1; a.width, a.height = 64, 48           # the grid alone: the keyframes are not read
        sc = bench.build_workload(a, log)
        g = bench.grid_arrays(sc); vs = float(np.float32(sc["voxel_size"]))
        surf, disp = surface_points(sc["scene"], a.points, np.random.default_rng(a.seed), vs)
        with binding.Context(0) as ctx:
            ctx.set_grid(vs, g["keys"], g["sdf"], g["sdf_refined"], g["albedo"], g["weight"], g["color"])
            fields = {"fused": dict(refined=False), "refined": dict(refined=True)}
            if a.refine_steps > 0:
                thres = a.shell * 2.0 * vs
                ctx.set_frames(sc["frames"], 1); ctx.set_camera(sc["intr"], sc["dist"], sc["poses"])
                ctx.estimate_sh(a.subvolume, 10.0, thres, cap=1 << 16)
                ctx.optimize(bench.make_cfg(binding, argparse.Namespace(pcg_fixed=-1, carry_radius=False), a.refine_steps, thres))
            out["context"] = {"voxels": int(g["keys"].shape[0]), "refine_steps": a.refine_steps, **leg(ctx.query_points, {"surface": surf, "displaced": disp}, vs, a.repeat, fields)}
    if not a.skip_fusion:
        from make_dataset import pose_vec_to_cam_to_world
        t0 = time.time()
        sc = synthetic.make_scene(radius_vox=a.fusion_radius, K=a.fusion_frames, width=640, height=480, levels=1, seed=1)
        log(f"fusion scene: {a.fusion_frames} frames rendered in {time.time() - t0:.1f}s")
        vs = float(np.float32(sc["voxel_size"])); intr = sc["intr"].astype(np.float32)
        with binding.Fusion(sc["voxel_size"], 0.1, 10.0, initial_capacity=1 << 24) as f:
            eyes = []
            for fr, p in zip(sc["frames"], sc["poses"]):
                T = pose_vec_to_cam_to_world(np.asarray(p, np.float64))
                f.integrate(fr["depth"][0], intr, fr["bgr"][0], intr, T.astype(np.float32), 2)
                eyes.append(T[:3, 3])
            e = eyes[0] - sc["scene"].c; e /= np.linalg.norm(e)     # the side the first frame saw
            surf, disp = surface_points(sc["scene"], a.points, np.random.default_rng(a.seed), vs, towards=e)
            res = {"before_finish": leg(f.query_points, {"surface": surf, "displaced": disp}, vs, a.repeat, {"fused": {}})}
            res["saved_voxels"] = int(f.finish(10))
            res["after_finish"] = leg(f.query_points, {"surface": surf}, vs, a.repeat, {"fused": {}})
            out["fusion"] = {"frames": a.fusion_frames, "radius_vox": a.fusion_radius, "points": int(surf.shape[0]), **res}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
