#!/usr/bin/env python3
"""Frame-to-model tracking during fusion (i3d_fusion_track) on fusion_bench.py's scene: a sphere of radius 302 voxels at 4 mm, 640x480
frames rendered by synthetic.render_frame along an arc (default 60 frames over 90 degrees), input poses carrying a seeded random walk (default 0.2 degrees and
1 voxel per frame; frame 0 exact).  Each frame after the first is registered against the volume fused so far from T_i0 = T_i,in T_j,in^-1 T_j,trk and
integrated at the result.  A second and a third volume are fused at the input poses and at the true poses.

    python tools/fusion_track_bench.py [--frames 60] [--arc-deg 90] [--sdf [--stride 1] [--huber-vox 0] [--rgbd [--photo-weight 0.1]]] [--repose]

--repose: after the tracked sequence, one leave-one-out pass over the tracked volume: every frame after the first is taken out
(i3d_fusion_deintegrate), registered against the rest by i3d_fusion_track_sdf from its tracked pose, and integrated at the result.  The trajectory error and the
held-out depth difference before and after the pass, the status counts and the host ms per frame of the three calls go under "repose".

--sdf fuses one more volume whose frames are registered on the volume's field itself, without a ray cast (i3d_fusion_track_sdf), from the
same input poses by the same chaining rule, in the same session; its figures go under "sdf" beside the ICP tracker's.

--sdf --rgbd fuses one more volume, on a textured scene (the same geometry and poses, the albedo of tests/fusion_track_sdf_rgbd_cases.py: the depth images are
the same, the colour images differ), whose frames are registered with the volume's fused colour beside its field (i3d_fusion_track_sdf_rgbd, DESIGN.md section
22).  On that volume every frame is also registered by i3d_fusion_track_sdf from the same guess, result discarded, the two calls timed in alternation; the
figures go under "sdf_rgbd": ms per frame of both, their ratio, and the trajectory error (the depth-only tracker's is "sdf"'s: it does not read the colour).

Prints one JSON line: host ms per frame of i3d_fusion_track, of i3d_fusion_integrate and of the brick bitmap rebuild (the first cast after an integrate, timed
with a 1x1 view), the status counts, the trajectory error (median / max, degrees and voxels) with tracking and of the raw input, and the median |depth
difference| of a held-out view cast from the tracked and from the untracked volume against the volume fused at the true poses, and the host ms of one view
cast from the true-pose volume's table and from a context that holds its export (the same volume, both casts).  The kernels' own times come
from a kernel trace of this command (rocprofv3 --kernel-trace --stats).
"""
import argparse, json, math, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from intrinsic3d_amd import binding, synthetic
import track_twin


def c2w(pose):
    R = synthetic.aa_to_rotmat(np.asarray(pose[:3], np.float64))
    T = np.eye(4); T[:3, :3] = R.T; T[:3, 3] = -R.T @ np.asarray(pose[3:], np.float64)
    return T.astype(np.float32)


def mat(p):
    M = np.eye(4); M[:3, :3] = synthetic.aa_to_rotmat(p[:3]); M[:3, 3] = p[3:]
    return M


def vec(M):
    return np.concatenate([synthetic.rotmat_to_aa(M[:3, :3]), M[:3, 3]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60); ap.add_argument("--arc-deg", type=float, default=90.0)
    ap.add_argument("--radius", type=int, default=302); ap.add_argument("--voxel-size", type=float, default=0.004)
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--walk-deg", type=float, default=0.2); ap.add_argument("--walk-vox", type=float, default=1.0); ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--sdf", action="store_true", help="also track with i3d_fusion_track_sdf into a volume of its own")
    ap.add_argument("--rgbd", action="store_true", help="with --sdf: also track with i3d_fusion_track_sdf_rgbd into a volume of its own, on a textured scene")
    ap.add_argument("--photo-weight", type=float, default=0.1)
    ap.add_argument("--repose", action="store_true", help="one leave-one-out pass over the tracked volume: deintegrate, track_sdf against the rest, integrate")
    ap.add_argument("--stride", type=int, default=1); ap.add_argument("--huber-vox", type=float, default=0.0, help="huber_delta in voxels (0: off)")
    a = ap.parse_args()
    if a.rgbd and not a.sdf:
        ap.error("--rgbd needs --sdf")
    vs, w, h, n = a.voxel_size, a.width, a.height, a.frames
    margin = int(np.ceil(a.radius + 3.2 + 4))
    scene = synthetic.Scene(np.full(3, (margin + 2) * vs), a.radius * vs, 0.5 * vs, 40.0)
    fx = 525.0 * w / 640.0
    intr = np.array([fx, fx, (w - 1) * 0.5, (h - 1) * 0.5]); intr32 = intr.astype(np.float32)
    dist = max(scene.R * fx / (0.35 * h), 2.5 * scene.R)

    def arc(th_deg, el_deg=15.0):
        th, el = math.radians(th_deg), math.radians(el_deg)
        return synthetic.look_at_pose(scene.c + dist * np.array([math.sin(th) * math.cos(el), math.sin(el), math.cos(th) * math.cos(el)]), scene.c)

    t0 = time.time()
    truth = [arc(a.arc_deg * i / max(1, n - 1)) for i in range(n)]
    rng = np.random.default_rng(a.seed)
    given = [np.asarray(truth[0], np.float64)]
    Rw, cw = np.eye(3), np.zeros(3)
    for i in range(1, n):
        ax = rng.normal(size=3); ax /= np.linalg.norm(ax); dt = rng.normal(size=3); dt /= np.linalg.norm(dt)
        Rw = synthetic.aa_to_rotmat(ax * math.radians(a.walk_deg)) @ Rw; cw = cw + dt * a.walk_vox * vs
        R = synthetic.aa_to_rotmat(truth[i][:3]); c = -R.T @ truth[i][3:]
        R2 = Rw @ R
        given.append(np.concatenate([synthetic.rotmat_to_aa(R2), -R2 @ (c + cw)]))
    frames = [synthetic.render_frame(scene, p, intr, w, h)[1:] for p in truth]
    textured, lums = [], []
    if a.rgbd:                                         # the same sphere with the textured albedo: only the colour images differ
        import fusion_track_sdf_rgbd_twin as FT
        tex = synthetic.Scene(scene.c, scene.R, scene.amp, scene.freq, albedo_freq=60.0, albedo_amp=0.3)
        textured = [synthetic.render_frame(tex, p, intr, w, h)[2] for p in truth]
        lums = [FT.frame_luminance(b, intr32, intr32, w, h) for b in textured]
    print(f"[fusion_track_bench] {n} frames {w}x{h} rendered in {time.time() - t0:.1f}s", file=sys.stderr)

    tiny = dict(width=1, height=1, intr=[1.0, 1.0, 0.0, 0.0], pose=truth[0])
    t_track, t_int, t_bits, status, tracked = [], [], [], {}, []
    t_sdf, status_sdf, tracked_sdf, its_sdf, its_icp = [], {}, [], [], []
    t_rgbd, t_rgbd_sdf, status_rgbd, tracked_rgbd, its_rgbd, samples_rgbd = [], [], {}, [], [], []
    vols = {m: binding.Fusion(vs, 0.1, 10.0, initial_capacity=1 << 25) for m in ("tracked", "given", "true") + (("sdf",) if a.sdf else ()) + (("sdf_rgbd",) if a.rgbd else ())}
    try:
        for i, (depth, bgr) in enumerate(frames):
            f = vols["tracked"]
            pose = given[i]
            if i > 0:
                guess = vec(mat(given[i]) @ np.linalg.inv(mat(given[i - 1])) @ mat(tracked[-1]))
                s = time.perf_counter(); f.render(camera=tiny, planes=("depth",)); t_bits.append(time.perf_counter() - s)
                s = time.perf_counter(); p, st = f.track(depth, guess, intr); t_track.append(time.perf_counter() - s)
                status[st["status"]] = status.get(st["status"], 0) + 1
                its_icp.append(st["iterations"][0])
                pose = p if st["status"] in (0, 1) else guess
            tracked.append(np.asarray(pose, np.float64))
            s = time.perf_counter(); f.integrate(depth, intr32, bgr, intr32, c2w(pose), 2); t_int.append(time.perf_counter() - s)
            if a.sdf:                                  # the same frame, the same chaining rule, the volume fused at the poses this tracker returned
                pose = given[i]
                if i > 0:
                    guess = vec(mat(given[i]) @ np.linalg.inv(mat(given[i - 1])) @ mat(tracked_sdf[-1]))
                    s = time.perf_counter(); p, st = vols["sdf"].track_sdf(depth, guess, intr, stride=a.stride, huber_delta=a.huber_vox * vs); t_sdf.append(time.perf_counter() - s)
                    status_sdf[st["status"]] = status_sdf.get(st["status"], 0) + 1
                    its_sdf.append(st["iterations"])
                    pose = p if st["status"] in (0, 1) else guess
                tracked_sdf.append(np.asarray(pose, np.float64))
                vols["sdf"].integrate(depth, intr32, bgr, intr32, c2w(pose), 2)
            if a.rgbd:                                 # the textured frame; on this volume the depth-only call runs too, from the same guess, for the time alone
                pose = given[i]
                if i > 0:
                    guess = vec(mat(given[i]) @ np.linalg.inv(mat(given[i - 1])) @ mat(tracked_rgbd[-1]))
                    kw = dict(stride=a.stride, huber_delta=a.huber_vox * vs)
                    s = time.perf_counter(); vols["sdf_rgbd"].track_sdf(depth, guess, intr, **kw); t_rgbd_sdf.append(time.perf_counter() - s)
                    s = time.perf_counter(); p, st = vols["sdf_rgbd"].track_sdf_rgbd(depth, lums[i], guess, intr, photo_weight=a.photo_weight, **kw)
                    t_rgbd.append(time.perf_counter() - s)
                    status_rgbd[st["status"]] = status_rgbd.get(st["status"], 0) + 1
                    its_rgbd.append(st["iterations"]); samples_rgbd.append(st["photo_samples"])
                    pose = p if st["status"] in (0, 1) else guess
                tracked_rgbd.append(np.asarray(pose, np.float64))
                vols["sdf_rgbd"].integrate(depth, intr32, textured[i], intr32, c2w(pose), 2)
            vols["given"].integrate(depth, intr32, bgr, intr32, c2w(given[i]), 2)
            vols["true"].integrate(depth, intr32, bgr, intr32, c2w(truth[i]), 2)
        held = dict(width=w, height=h, intr=intr, pose=arc(0.5 * a.arc_deg, 30.0))
        ref = vols["true"].render(camera=held)["depth"]

        def gap(m):
            d = vols[m].render(camera=held)["depth"]
            ok = (d > 0) & (ref > 0)
            return float(np.median(np.abs(d[ok] - ref[ok]))) / vs if ok.any() else None

        def err(ps):
            r = [track_twin.rot_err_deg(p, t) for p, t in zip(ps, truth)]; c = [track_twin.centre_err(p, t) / vs for p, t in zip(ps, truth)]
            return {"rot_deg_median": float(np.median(r)), "rot_deg_max": float(np.max(r)), "vox_median": float(np.median(c)), "vox_max": float(np.max(c))}

        gap_tracked = gap("tracked")                   # before any repose pass
        repose = None
        if a.repose:                                   # the tracked volume's frames have the ordinals 0 .. n-1
            f = vols["tracked"]
            before = {"tracked_error": err(tracked), "heldout_median_abs_ddepth_vox": gap_tracked}
            reposed, st_count, t_out, t_reg, t_in = [np.asarray(tracked[0], np.float64)], {}, [], [], []
            for i in range(1, n):
                depth, bgr = frames[i]
                fr = (depth, intr32, bgr, intr32)
                s = time.perf_counter(); f.deintegrate(i, *fr, c2w(tracked[i]), 2); t_out.append(time.perf_counter() - s)
                s = time.perf_counter(); p, st = f.track_sdf(depth, tracked[i], intr, stride=a.stride, huber_delta=a.huber_vox * vs); t_reg.append(time.perf_counter() - s)
                st_count[st["status"]] = st_count.get(st["status"], 0) + 1
                pose = np.asarray(p if st["status"] in (0, 1) else tracked[i], np.float64)
                reposed.append(pose)
                s = time.perf_counter(); f.integrate(*fr, c2w(pose), 2); t_in.append(time.perf_counter() - s)
            repose = {"before": before, "after": {"tracked_error": err(reposed), "heldout_median_abs_ddepth_vox": gap("tracked")},
                      "status": {str(k): v for k, v in sorted(st_count.items())}, "deintegrate_ms_per_frame": 1e3 * float(np.mean(t_out)),
                      "track_sdf_ms_per_frame": 1e3 * float(np.mean(t_reg)), "integrate_ms_per_frame": 1e3 * float(np.mean(t_in))}

        # one volume cast both ways (the table, and the context that loads its export), host ms per 640x480 view
        vols["true"].finish(0)
        ex = vols["true"].export()
        sd = ex["sdf"].astype(np.float64)
        def timed(fn, k=5):
            fn(); s = time.perf_counter()
            for _ in range(k):
                fn()
            return 1e3 * (time.perf_counter() - s) / k
        ms_fusion_cast = timed(lambda: vols["true"].render(camera=held))
        with binding.Context(0) as ctx:
            ctx.set_grid(vs, ex["keys"], sd, sd, np.zeros_like(sd), ex["weight"], ex["color"])
            ms_context_cast = timed(lambda: ctx.render_view(frame=-1, refined=False, planes=("depth", "normal"), camera=held))
        info = vols["tracked"].info()
        out = {"frames": n, "image": [w, h], "voxel_size": vs, "radius_vox": a.radius, "arc_deg": a.arc_deg,
               "track_ms_per_frame": 1e3 * float(np.mean(t_track[1:] if len(t_track) > 1 else t_track)),
               "integrate_ms_per_frame": 1e3 * float(np.mean(t_int[1:])), "bitmap_ms_per_frame": 1e3 * float(np.mean(t_bits[1:] if len(t_bits) > 1 else t_bits)),
               "status": {str(k): v for k, v in sorted(status.items())}, "tracked_error": err(tracked), "input_error": err(given),
               "heldout_median_abs_ddepth_vox": {"tracked": gap_tracked, "untracked": gap("given")}, "table_slots": info["capacity"],
               "allocated_true_volume": vols["true"].info()["allocated"], "cast_ms_fusion_table": ms_fusion_cast, "cast_ms_context_same_volume": ms_context_cast}
        if repose is not None:
            out["repose"] = repose
        out["track_mean_iterations"] = float(np.mean(its_icp)) if its_icp else None
        if a.sdf:
            out["sdf"] = {"stride": a.stride, "huber_vox": a.huber_vox, "track_ms_per_frame": 1e3 * float(np.mean(t_sdf[1:] if len(t_sdf) > 1 else t_sdf)),
                          "mean_iterations": float(np.mean(its_sdf)), "status": {str(k): v for k, v in sorted(status_sdf.items())}, "tracked_error": err(tracked_sdf),
                          "heldout_median_abs_ddepth_vox": gap("sdf")}
        if a.rgbd:
            mean = lambda t: 1e3 * float(np.mean(t[1:] if len(t) > 1 else t))  # noqa: E731
            out["sdf_rgbd"] = {"photo_weight": a.photo_weight, "track_ms_per_frame": mean(t_rgbd), "track_sdf_ms_per_frame_same_volume": mean(t_rgbd_sdf),
                               "ms_ratio": mean(t_rgbd) / mean(t_rgbd_sdf), "mean_iterations": float(np.mean(its_rgbd)), "mean_photo_samples": float(np.mean(samples_rgbd)),
                               "status": {str(k): v for k, v in sorted(status_rgbd.items())}, "tracked_error": err(tracked_rgbd),
                               "table_slots": vols["sdf_rgbd"].info()["capacity"], "heldout_median_abs_ddepth_vox": gap("sdf_rgbd")}
    finally:
        for f in vols.values():
            f.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
