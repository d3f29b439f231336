#!/usr/bin/env python3
"""Host cost of the context layer's calls, one library against another in one session (profiles/context_host_refactor.json).

    python tools/context_bench.py --libs parent=path/to/libparent.so change=intrinsic3d_amd/libintrinsic3d_hip.so [--rounds 5] [--voxels 1e6]

Measures the host milliseconds per call (wall clock around the binding's call: staging, launches, copies, the synchronisation) of set_grid, export_grid,
get_grid, update_grid, extract_mesh, clear_outside_thin_shell, upsample and set_frames_rgbd on the grid of `bench.py --voxels 1e6` (its build_workload; an
8 M-voxel grid would upsample to 64 M voxels, more than a timing needs) and --frames keyframes of 640 x 480 with a 3-level pyramid.

The binding loads one library per process, so every (library, round) is a child process of its own, started with I3D_LIB; the libraries take turns round by
round (sessions differ by about +-5 %, tools/ab_libs.sh: only same-session figures compare).  A child repeats the whole sequence --reps + 1 times (the
transitions change the grid, so every repetition starts from set_grid), drops the first as warm-up and reports the median of the rest.  Prints one JSON line: per
library and call the rounds' figures with their median, minimum and maximum, and per call whether the second library's median lies within the first's own
minimum-to-maximum spread."""
import argparse, json, os, statistics, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = ("set_grid", "export_grid", "get_grid", "update_grid", "extract_mesh", "clear_outside_thin_shell", "upsample", "set_frames_rgbd")


def child(a):
    from intrinsic3d_amd import binding
    d = np.load(a.child)
    g = [d[k] for k in ("keys", "sdf", "sdf_refined", "albedo", "weight", "color")]
    vs = float(d["voxel_size"]); bgr = list(d["bgr"]); depth = list(d["depth"])
    times = {k: [] for k in CALLS}

    def timed(name, fn):
        t0 = time.perf_counter(); out = fn(); times[name].append(1e3 * (time.perf_counter() - t0))
        return out
    sizes = {}
    with binding.Context(0) as ctx:
        for _ in range(a.reps + 1):
            timed("set_grid", lambda: ctx.set_grid(vs, *g))
            timed("export_grid", ctx.export_grid)
            sr, al = timed("get_grid", ctx.get_grid)
            timed("update_grid", lambda: ctx.update_grid(sr, al, g[5]))
            v, _, f = timed("extract_mesh", ctx.extract_mesh)
            sizes["mesh_faces"] = int(len(f))
            sizes["voxels_after_clear"] = int(timed("clear_outside_thin_shell", lambda: ctx.clear_outside_thin_shell(a.shell * 2.0 * vs)))
            sizes["voxels_after_upsample"] = int(timed("upsample", ctx.upsample))
            timed("set_frames_rgbd", lambda: ctx.set_frames_rgbd(bgr, depth, 3))
    print(json.dumps({"ms": {k: statistics.median(v[1:]) for k, v in times.items()}, "lib": binding.LIB_PATH, **sizes}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs=2, metavar="NAME=PATH", default=[]); ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--voxels", type=float, default=1.0e6); ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--width", type=int, default=640); ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--voxel-size", type=float, default=0.001); ap.add_argument("--band", type=float, default=3.5)
    ap.add_argument("--seed", type=int, default=1234); ap.add_argument("--shell", type=float, default=1.0)
    ap.add_argument("--timeout", type=int, default=120, help="seconds a child may take")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    import bench
    log = lambda m: print(f"[context_bench] {m}", file=sys.stderr)
    libs = [s.split("=", 1) for s in a.libs]
    assert len(libs) == 2 and all(os.path.exists(p) for _, p in libs), "two libraries: --libs parent=... change=..."
    sc = bench.build_workload(a, log)
    g = bench.grid_arrays(sc)
    rounds = {n: [] for n, _ in libs}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "workload.npz")
        np.savez(path, voxel_size=np.float32(sc["voxel_size"]), bgr=np.stack([f["bgr"][0] for f in sc["frames"]]), depth=np.stack([f["depth"][0] for f in sc["frames"]]), **g)
        for r in range(a.rounds):
            for name, lib in libs:
                # a child that fails or exceeds its limit ends the session: nothing more is started on a device that may have faulted
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--reps", str(a.reps), "--shell", str(a.shell)],
                                   env=dict(os.environ, I3D_LIB=os.path.abspath(lib)), capture_output=True, text=True, timeout=a.timeout)
                if p.returncode != 0:
                    sys.exit(f"context_bench: {name} round {r} failed ({p.returncode}):\n{p.stderr[-2000:]}")
                rounds[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
                log(f"round {r} {name}: " + ", ".join(f"{k} {v:.2f}" for k, v in rounds[name][-1]["ms"].items()))
    (base, _), (other, _) = libs
    out = {"voxels": int(g["keys"].shape[0]), "frames": a.frames, "image": [a.width, a.height], "pyramid_levels": 3, "rounds": a.rounds, "reps_per_round": a.reps,
           "sizes": {k: v for k, v in rounds[base][0].items() if k not in ("ms", "lib")}, "ms_per_call": {}, "verdict": {}}
    for name in (base, other):
        out["ms_per_call"][name] = {}
        for k in CALLS:
            v = [r["ms"][k] for r in rounds[name]]
            out["ms_per_call"][name][k] = {"rounds": [round(x, 4) for x in v], "median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    for k in CALLS:
        b, o = out["ms_per_call"][base][k], out["ms_per_call"][other][k]
        out["verdict"][k] = {f"{other}_median": o["median"], f"{base}_min": b["min"], f"{base}_max": b["max"], "within_spread": bool(b["min"] <= o["median"] <= b["max"]),
                             "median_ratio": round(o["median"] / b["median"], 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
