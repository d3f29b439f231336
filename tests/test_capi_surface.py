"""-m "not gpu": the C-ABI library loads and exports every symbol include/intrinsic3d_hip.h declares; host-side behaviour
that needs no device (defaults, error reporting, loud failure without a GPU)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from intrinsic3d_amd import binding
    if not os.path.exists(binding.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return binding, binding.load()


def test_every_declared_symbol_is_exported():
    binding, L = _lib()
    hdr = open(os.path.join(ROOT, "include", "intrinsic3d_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(i3d_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 25
    missing = [s for s in declared if not hasattr(L, s)]
    assert not missing, missing
    assert sorted(binding.EXPORTS) == declared


def test_struct_layouts_match_header():
    """ctypes mirrors must have the C struct sizes (checked against a tiny C program compiled with gcc)."""
    import ctypes, subprocess, tempfile
    binding, L = _lib()
    src = '#include <stdio.h>\n#include "intrinsic3d_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(i3d_optimizer_config), sizeof(i3d_iteration_stats), sizeof(i3d_grid_view), sizeof(i3d_sh_stats), sizeof(i3d_refine_config));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        sizes = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    assert sizes == [ctypes.sizeof(binding.OptimizerConfig), ctypes.sizeof(binding.IterationStats), ctypes.sizeof(binding.GridView), ctypes.sizeof(binding.ShStats),
                     ctypes.sizeof(binding.RefineConfig)]


def test_defaults_are_the_reference_struct_defaults():
    binding, L = _lib()
    c = binding.default_config()
    # optimizer.h:69-79 and intrinsic3d.h:72-80
    assert (c.iterations, c.lm_steps) == (10, 50)
    assert (c.lambda_g, c.lambda_r0, c.lambda_r1, c.lambda_s0, c.lambda_s1, c.lambda_a) == (0.2, 20.0, 160.0, 10.0, 120.0, 0.1)
    assert (c.fix_poses, c.fix_intrinsics, c.fix_distortion) == (0, 0, 0)
    assert abs(c.occlusion_distance - 0.02) < 1e-9 and c.num_observations == 5 and c.pcg_fixed_iterations == -1


def test_no_cpu_fallback_without_device():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    binding, L = _lib()
    if helpers.visible_devices() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(binding.I3DError) as e:
        binding.Context(0)
    assert "no CPU fallback" in str(e.value)


def test_product_never_imports_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline may touch oracle/."""
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "intrinsic3d_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".h")) or f == "Makefile":
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                if re.search(r"oracle_py|liboracle|i3d_oracle\.h|from oracle|import oracle|oracle/", txt):
                    bad.append(os.path.join(dirpath, f))
    assert not bad, bad


def test_bench_never_runs_fewer_ranks_than_asked_for():
    """`python bench.py --gpus 2` without a launcher starts its ranks itself; on a box with fewer devices (this container has none) it must exit non-zero
    with a message instead of reporting a one-rank run (round-2 review, item 2)."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    if helpers.visible_devices() >= 2:
        pytest.skip("this box can run two ranks")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--voxels", "1e5"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 2 and "refusing to run fewer ranks" in r.stderr and r.stdout.strip() == ""


def test_committed_counter_files_attach_to_the_bench_line():
    """bench.py takes roofline.traffic and roofline_build.valu_frac from the committed PMC / SQ passes when their kernel tag and workload match the run's:
    the files under profiles/ must match the current tag and the default workload, or the driver's bench line silently carries nulls."""
    import json
    sys.path.insert(0, ROOT)
    import bench
    d = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_default.json")))
    assert d["kernel_tag"] == bench.KERNEL_TAG
    rows, active = d["config"]["rows"]["Eg"], d["config"]["active_voxels"]
    for kernel in ("eg_mr2", "eg_mr3", "build"):
        t = bench.pmc_traffic(kernel, rows, active)
        assert t is not None and t[0] > 1e9 and t[1].startswith("r06_"), kernel
        s = bench.sq_valu(kernel, rows)
        assert s is not None and s["valu"] > 1e7 and s["source"].startswith("r06_"), kernel
    strict = 4.0 * (29 * rows + 7 * d["config"]["rows"]["Er"] + d["config"]["rows"]["Es"] + 2 * d["config"]["rows"]["Ea"])
    # one stream of the rows serves two / three systems: the measured bytes stay within ~1.2x of ONE system's strict bytes
    assert 1.05 < bench.pmc_traffic("eg_mr2", rows, active)[0] / strict < 1.25 and 1.05 < bench.pmc_traffic("eg_mr3", rows, active)[0] / strict < 1.30


def test_cpu_baseline_leg_times_the_collection_single_threaded_and_threaded():
    """bench.py's cpu_baseline leg (the oracle as the CHECKER / baseline, never the product) on a small scene: SURVEY section 8(d) asks for the residual collection
    timed on one thread, as the reference runs it, and threaded — the threaded walk must assemble the same rows.  (The device-parity part of the leg needs a GPU and
    reports None here.)"""
    import argparse
    import bench
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import helpers
    sc = helpers.small_scene(seed=4, radius_vox=12, K=6, width=96, height=72)
    sc = dict(sc); sc.setdefault("scene", None)
    args = argparse.Namespace(cpu_sample=4000, cpu_ref_sample=0, subvolume=0.05)
    out = bench.cpu_baseline(args, sc, 2.0 * float(sc["voxel_size"]), lambda m: None, device=0)
    assert out is not None and out["kind"] == "port" and out["value"] > 0
    ph = out["phases_s_per_iteration_sample"]; th = out["threaded_collection"]
    assert ph["collect_single_thread"] > 0 and ph["build_and_solve"] > 0
    assert th is not None and th["rows_equal_single_thread"] and th["collect_s"] > 0 and th["value"] > 0
