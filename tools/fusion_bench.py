#!/usr/bin/env python3
"""Throughput of the device TSDF fusion on the bench scene's frames (640x480, voxel 4 mm), with the CPU restatement timed on a few frames.

    python tools/fusion_bench.py --frames 40 --radius 302 [--cpu-frames 2] [--reintegrate [--rounds 3]] [--merge [--rounds 3]]

--reintegrate: before the volume is finished, every frame after the first is taken through one cycle, --rounds times over: deintegrate,
integrate, reintegrate to a pose one voxel away, and deintegrate + integrate back as two calls - the four timed in alternation in one session, host ms per call
with the synchronisation every call ends on.  The figures (median, quartiles) go under "reintegrate".

--merge: the frame list is split in two and each half fused into its own volume.  Then, --rounds times over in one session and in
alternation, each on a fresh volume of the first half: the aligned merge of the second half's volume (Fusion.merge, identity), a general merge under a seeded
motion of a few degrees and a few voxels, and integrating the second half's frames one by one - the only way to combine the halves without the merge.  Host ms
per call, with the session's ms per integrate beside them, under "merge".
"""
import argparse, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
from intrinsic3d_amd import binding, synthetic
from make_dataset import pose_vec_to_cam_to_world


def reintegrate_cycle(f, frames, intr, vs, rounds):
    """the four calls in alternation on the fused volume; every frame ends at the pose it started from"""
    ordinal = list(range(len(frames)))
    t = {"integrate": [], "deintegrate": [], "reintegrate": [], "deintegrate_plus_integrate": []}
    clock = time.perf_counter
    for r in range(rounds + 1):                                                      # round 0 warms up (the cells of the shifted poses are allocated there)
        for i in range(1, len(frames)):
            d, b, T = frames[i]
            T2 = T.copy(); T2[:3, 3] += np.float32(vs) * T[:3, 0]                    # one voxel along the camera's x axis
            fr = (d, intr, b, intr)
            s0 = clock(); f.deintegrate(ordinal[i], *fr, T, 2)
            s1 = clock(); o = f.integrate(*fr, T, 2)
            s2 = clock(); o = f.reintegrate(o, *fr, T, T2, 2)
            s3 = clock(); f.deintegrate(o, *fr, T2, 2); ordinal[i] = f.integrate(*fr, T, 2)
            s4 = clock()
            if r > 0:
                t["deintegrate"].append(s1 - s0); t["integrate"].append(s2 - s1); t["reintegrate"].append(s3 - s2); t["deintegrate_plus_integrate"].append(s4 - s3)
    q = lambda v: [round(1e3 * float(x), 4) for x in np.percentile(v, [25, 50, 75])]  # noqa: E731
    out = {"rounds": rounds, "calls_each": len(t["integrate"]), "table_slots": f.info()["capacity"]}
    for k, v in t.items():
        lo, mid, hi = q(v)
        out[k + "_ms"] = mid; out[k + "_ms_quartiles"] = [lo, hi]
    out["reintegrate_over_two_calls"] = out["reintegrate_ms"] / out["deintegrate_plus_integrate_ms"]
    return out


def merge_cycle(frames, intr, vs, rounds, capacity, seed=4):
    """aligned merge, general merge and frame-by-frame integration of the second half, each into a fresh volume of the first half, in alternation"""
    half = len(frames) // 2
    first, second = frames[:half], frames[half:]
    rng = np.random.default_rng(seed)
    axis = rng.normal(size=3); axis /= np.linalg.norm(axis)
    pose = np.concatenate([axis * np.radians(5.0), rng.uniform(-3.0, 3.0, 3) * vs])
    clock = time.perf_counter
    t = {"integrate": [], "merge_aligned": [], "merge_general": [], "integrate_second_half": []}
    stats = {}

    def fused(part, timed=None):
        f = binding.Fusion(vs, 0.1, 10.0, initial_capacity=capacity)
        for d, b, T in part:
            s0 = clock(); f.integrate(d, intr, b, intr, T, 2)
            if timed is not None:
                timed.append(clock() - s0)
        return f

    with fused(second) as src:
        for r in range(rounds + 1):                                                  # round 0 warms up (module load, the first allocations of every buffer)
            keep = r > 0
            with fused(first, t["integrate"] if keep else None) as f:
                s0 = clock(); st = f.merge(src); s1 = clock()
                if keep:
                    t["merge_aligned"].append(s1 - s0)
                stats["aligned"] = {k: st[k] for k in ("source_voxels", "sampled", "allocated", "aligned")}
            with fused(first) as f:
                s0 = clock(); st = f.merge(src, pose); s1 = clock()
                if keep:
                    t["merge_general"].append(s1 - s0)
                stats["general"] = {k: st[k] for k in ("source_voxels", "sampled", "allocated", "aligned")}
            with fused(first) as f:
                s0 = clock()
                for d, b, T in second:
                    f.integrate(d, intr, b, intr, T, 2)
                s1 = clock()
                if keep:
                    t["integrate_second_half"].append(s1 - s0)
                slots = f.info()["capacity"]
    q = lambda v: [round(1e3 * float(x), 4) for x in np.percentile(v, [25, 50, 75])]  # noqa: E731
    out = {"rounds": rounds, "frames_first": len(first), "frames_second": len(second), "table_slots": slots, "pose6": [float(x) for x in pose], "stats": stats}
    for k, v in t.items():
        lo, mid, hi = q(v)
        out[k + "_ms"] = mid; out[k + "_ms_quartiles"] = [lo, hi]
    out["merge_aligned_over_integrating"] = out["merge_aligned_ms"] / out["integrate_second_half_ms"]
    out["merge_general_over_integrating"] = out["merge_general_ms"] / out["integrate_second_half_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40); ap.add_argument("--radius", type=int, default=302)
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--cpu-frames", type=int, default=0); ap.add_argument("--correct", type=int, default=10)
    ap.add_argument("--reintegrate", action="store_true", help="time integrate / deintegrate / reintegrate / deintegrate + integrate in alternation")
    ap.add_argument("--merge", action="store_true", help="time the aligned merge, a general merge and integrating the second half's frames, in alternation")
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--workers", type=int, default=1, help="threads that render the frames")
    a = ap.parse_args()
    t0 = time.time()
    sc = synthetic.make_scene(radius_vox=a.radius, K=a.frames, width=a.width, height=a.height, levels=1, seed=1, workers=a.workers)
    intr = sc["intr"].astype(np.float32)
    frames = [(fr["depth"][0], fr["bgr"][0], pose_vec_to_cam_to_world(np.asarray(p, np.float64)).astype(np.float32)) for fr, p in zip(sc["frames"], sc["poses"])]
    print(f"[fusion_bench] {a.frames} frames {a.width}x{a.height} rendered in {time.time() - t0:.1f}s", file=sys.stderr)
    dmin, dmax = 0.1, 10.0
    with binding.Fusion(sc["voxel_size"], dmin, dmax, initial_capacity=1 << 25) as f:
        d, b, T = frames[0]; f.integrate(d, intr, b, intr, T, 2)                    # warm-up frame (module load, first allocations)
        t1 = time.time()
        for d, b, T in frames[1:]:
            f.integrate(d, intr, b, intr, T, 2)
        t2 = time.time()
        re = reintegrate_cycle(f, frames, intr, float(sc["voxel_size"]), a.rounds) if a.reintegrate else None
        t2b = time.time()
        mg = merge_cycle(frames, intr, float(sc["voxel_size"]), a.rounds, 1 << 25) if a.merge else None
        t2b = time.time()
        n = f.finish(a.correct)
        t3 = time.time()
        info = f.info()
    out = {"frames": a.frames, "image": [a.width, a.height], "voxel_size": float(sc["voxel_size"]), "ms_per_frame": 1e3 * (t2 - t1) / max(1, a.frames - 1),
           "finish_s": t3 - t2b, "allocated": info["allocated"], "saved": n, "table_slots": info["capacity"], "correct_launches": info["correct_launches"]}
    if re is not None:
        out["reintegrate"] = re
    if mg is not None:
        out["merge"] = mg
    if a.cpu_frames > 0:
        from oracle import oracle_py as O
        O.build()
        o = O.Fusion(sc["voxel_size"], dmin, dmax)
        t4 = time.time()
        for d, b, T in frames[:a.cpu_frames]:
            o.integrate(d, intr, b, intr, T, 2)
        out["cpu_ms_per_frame"] = 1e3 * (time.time() - t4) / a.cpu_frames; out["cpu_frames"] = a.cpu_frames
    print(json.dumps(out))


if __name__ == "__main__":
    main()
