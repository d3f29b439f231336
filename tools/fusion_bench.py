#!/usr/bin/env python3
"""Throughput of the device TSDF fusion on the bench scene's frames (640x480, voxel 4 mm), with the CPU restatement timed on a few frames.

    python tools/fusion_bench.py --frames 40 --radius 302 [--cpu-frames 2] [--reintegrate [--rounds 3]] [--merge [--rounds 3]] [--register-volume [--rounds 3]] [--mesh] [--load [--rounds 3]] [--prune [--rounds 3]] [--components [--rounds 3]]

--reintegrate: before the volume is finished, every frame after the first is taken through one cycle, --rounds times over: deintegrate,
integrate, reintegrate to a pose one voxel away, and deintegrate + integrate back as two calls - the four timed in alternation in one session, host ms per call
with the synchronisation every call ends on.  The figures (median, quartiles) go under "reintegrate".

--merge: the frame list is split in two and each half fused into its own volume.  Then, --rounds times over in one session and in
alternation, each on a fresh volume of the first half: the aligned merge of the second half's volume (Fusion.merge, identity), a general merge under a seeded
motion of a few degrees and a few voxels, and integrating the second half's frames one by one - the only way to combine the halves without the merge.  Host ms
per call, with the session's ms per integrate beside them, under "merge".

--register-volume: the frame list is split in two, on depth images of a sphere whose bumps make a rotation observable (2 voxels at a
wavelength of 16; the bench scene's own depth is the smooth sphere's).  The second half is fused at poses moved by a seeded rigid motion, so that its world differs
from the first's by a known T.  Then, --rounds times over in one session and in alternation on the same two volumes, from one perturbed start: (a)
Fusion.register_volume; (b) the route there was before - points near the second volume's surface (its frames' depth pixels, every fourth in each direction, taken
to its world before the clock starts) walked onto its zero level by Fusion.query_points(project=1), the feet registered by Fusion.register_points, timed with the
host work between the two calls; (c) Fusion.merge under the pose (a) found, into a fresh volume of the first half.  (a) is repeated at source_band_voxels 1, 2, 3
and stride 1, 2.  Host ms per call with the call's own synchronisations, iterations, counts and the pose error against T, under "register_volume" and in
profiles/fusion_register_volume.json.

--mesh: on the finished volume, 5 rounds in one session and in alternation (after one untimed round of each): (a) Fusion.extract_mesh; (b) the
route to a mesh there was before - export(), Context.set_grid in record order, Context.extract_mesh(False, 0, False).  Host ms per route with each call's own
synchronisations, medians and quartiles, vertex and face counts, under "mesh" and in profiles/fusion_mesh.json.

--load: --rounds times over in one session and in alternation (after one untimed round): the frames fused into a fresh volume, snapshot()
twice (the first also grows the handle's slot list), save(), finish(0) on that same volume, and Fusion.load of the saved file into a fresh volume.  Host ms per
call with each call's own synchronisations, medians and quartiles, under "load" and in profiles/fusion_load.json.

--prune: --rounds times over in one session and in alternation (after one untimed round), each on a fresh volume of the frames: (a)
Fusion.prune() with its defaults (the weightless voxels leave, the capacity stays); (b) the route there was before - snapshot(), export(), the filter on the host,
a new handle, insert_records(); (c) one integrate before a prune and the same frame once more after prune(shrink=True), with that prune timed as well.  Host ms per
call with each call's own synchronisations, medians and quartiles, the counts and the capacities, under "prune" and in profiles/fusion_prune.json.
--components: --rounds times over in one session and in alternation (after one untimed round), each on a fresh volume of the frames with a
few hundred seeded blobs cut loose in it (the shell of a 5x5x5 cube around a seeded stored voxel poked to weight 0: the 27 voxels inside are a floater): (a)
Fusion.components(); (b) Fusion.prune_components(min_voxels=64) on the same volume; (c) Fusion.prune() with its defaults on such a volume; (d) extract_mesh() and
extract_mesh(largest_component_only=True), whose difference is the component cost of the host route.  Host ms per call with each call's own synchronisations,
medians and quartiles and the counts, under "components" and in profiles/fusion_components.json.
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


def bumpy_depth(scene, pose6, intr, w, h, iters=60):
    """z-depth of the bumpy sphere along the pixel rays of render_frame's camera: damped sphere tracing from the bounding sphere, 0 where the ray misses"""
    fx, fy, cx, cy = intr
    R = synthetic.aa_to_rotmat(pose6[:3]); eye = -R.T @ pose6[3:]
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    dw = (np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1) @ R).reshape(-1, 3)
    oc = eye - scene.c
    qa = (dw * dw).sum(-1); qb = 2.0 * (dw @ oc); qc = oc @ oc - (scene.R + 2.0 * abs(scene.amp)) ** 2
    disc = qb * qb - 4 * qa * qc
    live = np.nonzero(disc > 0)[0]
    d = dw[live]; t = np.maximum((-qb[live] - np.sqrt(disc[live])) / (2 * qa[live]), 0.0)
    step = 0.9 / ((1.0 + abs(scene.amp) * scene.freq * np.sqrt(3.0)) * np.sqrt(qa[live]))
    for _ in range(iters):
        t = t + step * scene.sdf(eye + t[:, None] * d)
    hit = np.abs(scene.sdf(eye + t[:, None] * d)) < 1e-7
    depth = np.zeros(w * h, np.float32); depth[live[hit]] = t[hit]
    return depth.reshape(h, w)


def pose_error(a, b, vs):
    """(rotation angle between two angle-axis | t poses in degrees, |t_a - t_b| in voxels)"""
    D = synthetic.aa_to_rotmat(np.asarray(a[:3], np.float64)) @ synthetic.aa_to_rotmat(np.asarray(b[:3], np.float64)).T
    sk = 0.5 * np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    return float(np.degrees(np.arctan2(np.sqrt((sk * sk).sum()), 0.5 * (np.trace(D) - 1.0)))), float(np.linalg.norm(np.asarray(a[3:]) - np.asarray(b[3:])) / vs)


def register_volume_cycle(sc, rounds, capacity, seed=6, pixel_step=4):
    """register_volume, the query + register_points route and the merge under the pose found, in alternation on two volumes whose worlds differ by a known T"""
    vs = float(sc["voxel_size"]); intr = sc["intr"].astype(np.float32); w, h = sc["width"], sc["height"]
    scene = synthetic.Scene(sc["center"], sc["scene"].R, 2.0 * vs, 2.0 * np.pi / (16.0 * vs))
    K = len(sc["poses"]); half = K // 2
    rng = np.random.default_rng(seed)

    def about_centre(deg, vox):
        axis = rng.normal(size=3); axis *= np.radians(deg) / np.linalg.norm(axis)
        shift = rng.normal(size=3); shift *= vox * vs / np.linalg.norm(shift)
        return synthetic.aa_to_rotmat(axis), shift

    R, shift = about_centre(5.0, 3.0)
    t = scene.c - R @ scene.c + shift
    T = np.concatenate([synthetic.rotmat_to_aa(R), t])
    Tm = np.eye(4); Tm[:3, :3] = R; Tm[:3, 3] = t; Tinv = np.linalg.inv(Tm)
    dR, du = about_centre(0.5, 1.0)
    start = np.concatenate([synthetic.rotmat_to_aa(dR @ R), dR @ (t - scene.c) + scene.c + du])
    t0 = time.time()
    first, second, seeds = [], [], []
    for i, (fr, p) in enumerate(zip(sc["frames"], sc["poses"])):
        p = np.asarray(p, np.float64); d = bumpy_depth(scene, p, sc["intr"], w, h); c2w = pose_vec_to_cam_to_world(p)
        if i < half:
            first.append((d, fr["bgr"][0], c2w.astype(np.float32)))
        else:
            moved = Tinv @ c2w
            second.append((d, fr["bgr"][0], moved.astype(np.float32)))
            v, u = np.nonzero(d[::pixel_step, ::pixel_step] > 0); z = d[::pixel_step, ::pixel_step][v, u].astype(np.float64)
            cam = np.stack([(u * pixel_step - sc["intr"][2]) / sc["intr"][0] * z, (v * pixel_step - sc["intr"][3]) / sc["intr"][1] * z, z], -1)
            seeds.append(cam @ moved[:3, :3].T + moved[:3, 3])
    seeds = np.ascontiguousarray(np.concatenate(seeds))
    print(f"[fusion_bench] {K} bumpy depth images traced in {time.time() - t0:.1f}s; {len(seeds)} seed points", file=sys.stderr)

    def fused(part):
        f = binding.Fusion(vs, 0.1, 10.0, initial_capacity=capacity)
        for d, b, c2w in part:
            f.integrate(d, intr, b, intr, c2w, 2)
        return f

    clock = time.perf_counter
    variants = [(band, stride) for band in (1.0, 2.0, 3.0) for stride in (1, 2)]
    t = {"register_volume": [], "query_plus_register_points": [], "merge": []}
    tv = {v: [] for v in variants}
    res = {}
    with fused(first) as A, fused(second) as src:
        for r in range(rounds + 1):                                                  # round 0 warms up (module load, the first allocations of every scratch)
            keep = r > 0
            s0 = clock(); pa, sa = A.register_volume(src, start); s1 = clock()
            q = src.query_points(seeds, outputs=("foot", "status"), project=1)
            feet = np.ascontiguousarray(q["foot"][(q["status"] & 2) != 0])
            pb, sb = A.register_points(feet, start); s2 = clock()
            with fused(first) as fresh:
                s3 = clock(); ms = fresh.merge(src, pa); s4 = clock()
            if keep:
                t["register_volume"].append(s1 - s0); t["query_plus_register_points"].append(s2 - s1); t["merge"].append(s4 - s3)
            for band, stride in variants:
                s5 = clock(); pv, sv = A.register_volume(src, start, source_band_voxels=band, stride=stride); s6 = clock()
                if keep:
                    tv[(band, stride)].append(s6 - s5)
                res[(band, stride)] = (pv, sv)
        slots = (A.info()["capacity"], src.info()["capacity"])
    q3 = lambda v: [round(1e3 * float(x), 4) for x in np.percentile(v, [25, 50, 75])]  # noqa: E731

    def figures(pose, st, extra=()):
        deg, vox = pose_error(pose, T, vs)
        return dict({k: st[k] for k in ("status", "iterations", "valid", "inliers", "rms_initial", "rms_final") + tuple(extra)}, error_deg=deg, error_voxels=vox)

    d0, v0 = pose_error(start, T, vs)
    out = {"rounds": rounds, "frames_first": len(first), "frames_second": len(second), "table_slots": slots, "T": [float(x) for x in T], "start": [float(x) for x in start],
           "start_error_deg": d0, "start_error_voxels": v0, "seed_points": int(len(seeds)), "feet": int(len(feet)),
           "register_volume": figures(pa, sa, ("selected",)), "query_plus_register_points": figures(pb, sb),
           "merge": {k: ms[k] for k in ("source_voxels", "sampled", "allocated", "aligned")}}
    for k, v in t.items():
        lo, mid, hi = q3(v)
        out[k + "_ms"] = mid; out[k + "_ms_quartiles"] = [lo, hi]
    out["register_volume_over_points_route"] = out["register_volume_ms"] / out["query_plus_register_points_ms"]
    out["variants"] = []
    for (band, stride), v in tv.items():
        lo, mid, hi = q3(v)
        out["variants"].append(dict(figures(*res[(band, stride)], ("selected",)), source_band_voxels=band, stride=stride, ms=mid, ms_quartiles=[lo, hi]))
    return out


def mesh_cycle(f, vs, rounds=5):
    """Fusion.extract_mesh against export + Context.set_grid + Context.extract_mesh on the finished volume f, in alternation"""
    clock = time.perf_counter
    t = {"fusion_extract_mesh": [], "context_route": [], "context_route_export": [], "context_route_set_grid": [], "context_route_extract_mesh": []}
    out = {"rounds": rounds}
    for r in range(rounds + 1):                                                      # round 0 warms up (scratch buffers, module load)
        s0 = clock(); v, c, fc, st = f.extract_mesh(stats=True)
        s1 = clock(); ex = f.export()
        s2 = clock()
        with binding.Context() as ctx:
            ctx.set_grid(vs, ex["keys"], ex["sdf"], ex["sdf"], np.zeros(len(ex["sdf"])), ex["weight"], ex["color"])
            s3 = clock(); rv, rc, rf = ctx.extract_mesh(False, 0, False)
            s4 = clock()
        if r > 0:
            t["fusion_extract_mesh"].append(s1 - s0); t["context_route"].append(s4 - s1); t["context_route_export"].append(s2 - s1)
            t["context_route_set_grid"].append(s3 - s2); t["context_route_extract_mesh"].append(s4 - s3)
        out.update(stats=st, vertices=len(v), faces=len(fc), context_route_vertices=len(rv), context_route_faces=len(rf))
    q = lambda x: [round(1e3 * float(y), 4) for y in np.percentile(x, [25, 50, 75])]  # noqa: E731
    for k, x in t.items():
        lo, mid, hi = q(x)
        out[k + "_ms"] = mid; out[k + "_ms_quartiles"] = [lo, hi]
    out["fusion_over_context_route"] = out["fusion_extract_mesh_ms"] / out["context_route_ms"]
    return out


def load_cycle(frames, intr, vs, rounds, capacity):
    """Fusion.load of the saved volume against re-fusing its frames, and snapshot against finish(0) on a copy (the re-fused volume), in alternation"""
    import tempfile
    clock = time.perf_counter
    t = {"load": [], "refuse_frames": [], "snapshot_first": [], "snapshot": [], "finish0": [], "save": []}
    out = {"rounds": rounds, "frames": len(frames)}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "volume.tsdf")
        for r in range(rounds + 1):                                                  # round 0 warms up (module load, the first allocations) and writes the file
            keep = r > 0
            s0 = clock()
            f = binding.Fusion(vs, 0.1, 10.0, initial_capacity=capacity)
            for d, b, T in frames:
                f.integrate(d, intr, b, intr, T, 2)
            s1 = clock(); f.snapshot()                                                # the first one on a volume also grows the handle's slot list ...
            s1b = clock(); n = f.snapshot()                                           # ... which this one and the finish below find grown: these two are compared
            s2 = clock(); f.save(path)
            s3 = clock(); m = f.finish(0)
            s4 = clock()
            out.update(saved=int(n), allocated=int(f.info()["allocated"]), table_slots=int(f.info()["capacity"]), file_bytes=os.path.getsize(path))
            assert m == n
            f.close()
            s5 = clock()
            with binding.Fusion.load(path, 0.1, 10.0) as g:
                s6 = clock()
                out["loaded_table_slots"] = int(g.info()["capacity"])
            if keep:
                t["refuse_frames"].append(s1 - s0); t["snapshot_first"].append(s1b - s1); t["snapshot"].append(s2 - s1b); t["save"].append(s3 - s2); t["finish0"].append(s4 - s3); t["load"].append(s6 - s5)
    q = lambda v: [round(1e3 * float(x), 4) for x in np.percentile(v, [25, 50, 75])]  # noqa: E731
    for k, v in t.items():
        lo, mid, hi = q(v)
        out[k + "_ms"] = mid; out[k + "_ms_quartiles"] = [lo, hi]
    out["load_over_refusing"] = out["load_ms"] / out["refuse_frames_ms"]
    out["snapshot_over_finish0"] = out["snapshot_ms"] / out["finish0_ms"]
    return out


def prune_cycle(frames, intr, vs, rounds, capacity):
    """Fusion.prune with its defaults against snapshot + export + filter + insert_records, and an integrate before and after a shrinking prune, in alternation"""
    clock = time.perf_counter
    t = {"prune": [], "host_route": [], "host_route_snapshot": [], "host_route_export": [], "host_route_insert_records": [], "integrate_before": [], "prune_shrink": [],
         "integrate_after_shrink": []}
    out = {"rounds": rounds, "frames": len(frames)}

    def fused(part):
        f = binding.Fusion(vs, 0.1, 10.0, initial_capacity=capacity)
        for d, b, T in part:
            f.integrate(d, intr, b, intr, T, 2)
        return f

    d, b, T = frames[-1]
    for r in range(rounds + 1):                                                      # round 0 warms up (module load, the first allocations)
        keep = r > 0
        with fused(frames) as f:
            s0 = clock(); c = f.prune(); s1 = clock()
            out.update(counts=c, table_slots=int(f.info()["capacity"]))
        with fused(frames) as f:
            s2 = clock(); f.snapshot()
            s3 = clock(); ex = f.export()
            s4 = clock(); on = ex["weight"] > 0                                       # the filter: here the one snapshot has already applied
            with binding.Fusion(vs, 0.1, 10.0, initial_capacity=capacity) as g:
                g.insert_records(ex["keys"][on], ex["sdf"][on], ex["weight"][on], ex["color"][on])
                s5 = clock()
                out["host_route_records"] = int(on.sum())
        with fused(frames[:-1]) as f:
            s6 = clock(); f.integrate(d, intr, b, intr, T, 2)
            s7 = clock(); cs = f.prune(shrink=True)
            s8 = clock(); f.integrate(d, intr, b, intr, T, 2)
            s9 = clock()
            out.update(counts_shrink=cs, table_slots_after_shrink_and_integrate=int(f.info()["capacity"]))
        if keep:
            t["prune"].append(s1 - s0); t["host_route"].append(s5 - s2); t["host_route_snapshot"].append(s3 - s2); t["host_route_export"].append(s4 - s3)
            t["host_route_insert_records"].append(s5 - s4); t["integrate_before"].append(s7 - s6); t["prune_shrink"].append(s8 - s7); t["integrate_after_shrink"].append(s9 - s8)
    q = lambda v: [round(1e3 * float(x), 4) for x in np.percentile(v, [25, 50, 75])]  # noqa: E731
    for k, v in t.items():
        lo, mid, hi = q(v)
        out[k + "_ms"] = mid; out[k + "_ms_quartiles"] = [lo, hi]
    out["prune_over_host_route"] = out["prune_ms"] / out["host_route_ms"]
    out["integrate_after_over_before"] = out["integrate_after_shrink_ms"] / out["integrate_before_ms"]
    return out


def components_cycle(frames, intr, vs, rounds, capacity, blobs=300, seed=5):
    """Fusion.components and Fusion.prune_components against Fusion.prune and against the component pass of the host's mesh route, in alternation"""
    clock = time.perf_counter
    t = {"components": [], "prune_components": [], "prune": [], "extract_mesh": [], "extract_mesh_largest": []}
    out = {"rounds": rounds, "frames": len(frames), "blobs": blobs, "min_voxels": 64}
    cube = np.stack(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    shell = cube[np.abs(cube).max(1) == 2]
    state = {}

    def fused():
        f = binding.Fusion(vs, 0.1, 10.0, initial_capacity=capacity)
        for d, b, T in frames:
            f.integrate(d, intr, b, intr, T, 2)
        if not state:                                                             # the centres, once: seeded picks among the weighted voxels
            f.snapshot(); ex = f.export()
            pick = np.random.default_rng(seed).choice(len(ex["sdf"]), blobs, replace=False)
            k = np.unique((ex["keys"][pick].astype(np.int64)[:, None, :] + shell[None]).reshape(-1, 3), axis=0).astype(np.int32)
            state.update(keys=np.ascontiguousarray(k), zero=np.zeros(len(k), np.float32), color=np.zeros((len(k), 3), np.uint8))
        found = f.debug_poke_voxels(state["keys"], state["zero"], state["zero"], state["color"])
        out["shell_voxels_poked"] = int(found.sum())
        return f

    for r in range(rounds + 1):                                                      # round 0 warms up (module load, the first allocations, the grown-only buffers)
        keep = r > 0
        with fused() as f:
            s0 = clock(); c = f.components()
            s1 = clock(); pc = f.prune_components(min_voxels=out["min_voxels"])
            s2 = clock()
            out.update(nodes=c["nodes"], components=c["components"], largest=c["largest"], sizes_head=c["sizes"][:8].tolist(), prune_components_counts=pc,
                       table_slots=int(f.info()["capacity"]))
        with fused() as f:
            s3 = clock(); p = f.prune(); s4 = clock()
            out["prune_counts"] = p
        with fused() as f:
            s5 = clock(); v, _, fc = f.extract_mesh()
            s6 = clock(); lv, _, lf = f.extract_mesh(largest_component_only=True)
            s7 = clock()
            out.update(mesh_vertices=len(v), mesh_faces=len(fc), largest_mesh_vertices=len(lv), largest_mesh_faces=len(lf))
        if keep:
            t["components"].append(s1 - s0); t["prune_components"].append(s2 - s1); t["prune"].append(s4 - s3); t["extract_mesh"].append(s6 - s5)
            t["extract_mesh_largest"].append(s7 - s6)
    q = lambda v: [round(1e3 * float(x), 4) for x in np.percentile(v, [25, 50, 75])]  # noqa: E731
    for k, v in t.items():
        lo, mid, hi = q(v)
        out[k + "_ms"] = mid; out[k + "_ms_quartiles"] = [lo, hi]
    out["host_mesh_component_pass_ms"] = out["extract_mesh_largest_ms"] - out["extract_mesh_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40); ap.add_argument("--radius", type=int, default=302)
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--cpu-frames", type=int, default=0); ap.add_argument("--correct", type=int, default=10)
    ap.add_argument("--reintegrate", action="store_true", help="time integrate / deintegrate / reintegrate / deintegrate + integrate in alternation")
    ap.add_argument("--merge", action="store_true", help="time the aligned merge, a general merge and integrating the second half's frames, in alternation")
    ap.add_argument("--register-volume", action="store_true", help="time Fusion.register_volume against query_points + register_points, and the merge under its pose")
    ap.add_argument("--mesh", action="store_true", help="time Fusion.extract_mesh against export + Context.set_grid + Context.extract_mesh on the finished volume")
    ap.add_argument("--load", action="store_true", help="time Fusion.load of the saved volume against re-fusing its frames, and snapshot against finish(0)")
    ap.add_argument("--prune", action="store_true", help="time Fusion.prune against snapshot + export + insert_records, and an integrate before and after a shrinking prune")
    ap.add_argument("--components", action="store_true", help="time Fusion.components and Fusion.prune_components against Fusion.prune and the host mesh route's component pass")
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
        rv = register_volume_cycle(sc, a.rounds, 1 << 25) if a.register_volume else None
        ld = load_cycle(frames, intr, float(sc["voxel_size"]), a.rounds, 1 << 25) if a.load else None
        pr = prune_cycle(frames, intr, float(sc["voxel_size"]), a.rounds, 1 << 25) if a.prune else None
        cp = components_cycle(frames, intr, float(sc["voxel_size"]), a.rounds, 1 << 25) if a.components else None
        t2b = time.time()
        n = f.finish(a.correct)
        t3 = time.time()
        info = f.info()
        ms = mesh_cycle(f, float(sc["voxel_size"])) if a.mesh else None
    out = {"frames": a.frames, "image": [a.width, a.height], "voxel_size": float(sc["voxel_size"]), "ms_per_frame": 1e3 * (t2 - t1) / max(1, a.frames - 1),
           "finish_s": t3 - t2b, "allocated": info["allocated"], "saved": n, "table_slots": info["capacity"], "correct_launches": info["correct_launches"]}
    if re is not None:
        out["reintegrate"] = re
    if mg is not None:
        out["merge"] = mg
    if rv is not None:
        out["register_volume"] = rv
        with open(os.path.join(ROOT, "profiles", "fusion_register_volume.json"), "w") as fh:
            fh.write(json.dumps(out) + "\n")
    if ld is not None:
        out["load"] = ld
        with open(os.path.join(ROOT, "profiles", "fusion_load.json"), "w") as fh:
            fh.write(json.dumps(out) + "\n")
    if pr is not None:
        out["prune"] = pr
        with open(os.path.join(ROOT, "profiles", "fusion_prune.json"), "w") as fh:
            fh.write(json.dumps(out) + "\n")
    if cp is not None:
        out["components"] = cp
        with open(os.path.join(ROOT, "profiles", "fusion_components.json"), "w") as fh:
            fh.write(json.dumps(out) + "\n")
    if ms is not None:
        out["mesh"] = ms
        with open(os.path.join(ROOT, "profiles", "fusion_mesh.json"), "w") as fh:
            fh.write(json.dumps(out) + "\n")
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
