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


def _header():
    """include/intrinsic3d_hip.h without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "intrinsic3d_hip.h")).read(), flags=re.S)


def _mirrors():
    """{C name: ctypes mirror} of every struct abi.py mirrors, found through _c_name_"""
    import ctypes
    from intrinsic3d_amd import abi
    return {v._c_name_: v for v in vars(abi).values() if isinstance(v, type) and issubclass(v, ctypes.Structure) and "_c_name_" in vars(v)}


def test_struct_layouts_match_header():
    """Every ctypes mirror has its C struct's size and every field its C offset (a C program compiled with gcc prints both); so has the numpy record of
    i3d_lm_record."""
    import ctypes, subprocess, tempfile
    binding, L = _lib()
    mirrors = _mirrors()
    declared = set(re.findall(r"\}\s*(i3d_[a-z0-9_]+)\s*;", _header())) - {"i3d_status"}
    assert len(mirrors) == 25 and set(mirrors) == declared - {"i3d_lm_record"}
    layouts = {name: [k for k, _ in m._fields_] for name, m in mirrors.items()}
    layouts["i3d_lm_record"] = list(binding.LM_RECORD_DTYPE.names)
    items = list(layouts) + [n + "." + k for n, ks in layouts.items() for k in ks]
    body = "".join('printf("%s %%zu\\n", %s);\n' % (it, "offsetof(%s, %s)" % tuple(it.split(".")) if "." in it else "sizeof(%s)" % it) for it in items)
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "intrinsic3d_hip.h"\nint main(){\n' + body + "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        c = {k: int(v) for k, v in (ln.split() for ln in subprocess.check_output([os.path.join(d, "t")], text=True).splitlines())}
    py = {}
    for name, m in mirrors.items():
        py[name] = ctypes.sizeof(m)
        py.update({name + "." + k: getattr(m, k).offset for k, _ in m._fields_})
    rec = binding.LM_RECORD_DTYPE
    py["i3d_lm_record"] = rec.itemsize
    py.update({"i3d_lm_record." + k: rec.fields[k][1] for k in rec.names})
    assert len(c) == len(py) > 250
    assert {k: (c[k], py[k]) for k in c if c[k] != py[k]} == {}
    assert [c[n] for n in ("i3d_optimizer_config", "i3d_iteration_stats", "i3d_grid_view", "i3d_sh_stats", "i3d_refine_config")] == \
        [ctypes.sizeof(binding.OptimizerConfig), ctypes.sizeof(binding.IterationStats), ctypes.sizeof(binding.GridView), ctypes.sizeof(binding.ShStats),
         ctypes.sizeof(binding.RefineConfig)]


def test_prototypes_match_header():
    """abi.PROTOTYPES against the declarations of the header: the same functions, and for each the declared number of parameters, every parameter and the return
    value of the declared kind (pointer, float, double, 32- or 64-bit integer by signedness).  Reads the table; loads nothing."""
    import ctypes as C
    from intrinsic3d_amd import abi
    hdr = _header()
    callbacks = set(re.findall(r"typedef\s+\w+\s*\(\s*\*\s*(\w+)\s*\)", hdr))
    assert callbacks == {"i3d_refine_callback"}
    scalar = {"float": C.c_float, "double": C.c_double, "int": C.c_int32, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}

    def is_pointer(t):
        return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, (C._Pointer, C._CFuncPtr)))

    declared = {}
    for stmt in hdr.split(";"):
        stmt = " ".join(stmt.split())
        if not re.search(r"\bi3d_[a-z0-9_]+ ?\(", stmt):
            continue
        m = re.fullmatch(r"([\w \*]+?) ?\b(i3d_[a-z0-9_]+) ?\(([^()]*)\)", stmt)
        assert m, stmt                                                        # a declaration this parser cannot read fails, it is not skipped
        ret, name, params = m.group(1).strip(), m.group(2), [p.strip() for p in m.group(3).split(",")]
        assert name not in declared, name
        declared[name] = (ret, [] if params == ["void"] else params)
    table = {name: (restype, argtypes) for name, restype, argtypes in abi.PROTOTYPES}
    assert len(table) == len(abi.PROTOTYPES) and list(table) == list(declared)            # no double entry; the header's functions in the header's order
    assert abi.EXPORTS == list(declared) and len(declared) >= 148
    bad = []
    for name, (ret, params) in declared.items():
        restype, argtypes = table[name]
        if "*" in ret:
            ok = restype in (C.c_char_p, C.c_void_p)
        elif ret == "void":
            ok = restype is None
        else:
            ok = restype is scalar[ret] and ret in ("int", "int32_t", "int64_t")          # KeyError: a return type this test does not know
        if not ok:
            bad.append((name, "returns", ret, restype))
        if len(params) != len(argtypes):
            bad.append((name, "parameters", len(params), len(argtypes)))
            continue
        for p, t in zip(params, argtypes):
            words = [w for w in re.sub(r"[\*\[\]]", " ", p).split() if w != "const"]
            if "*" in p or "[" in p or words[0] in callbacks:
                ok = is_pointer(t)
            else:
                ok = t is scalar[words[0]]                                     # KeyError: a parameter type this test does not know
            if not ok:
                bad.append((name, p, t))
    assert not bad, bad


# name of the builder: (struct, aliases it takes {keyword: field}); the *_rgbd builders hand everything but their three own fields to the builder of `base`
DESC_BUILDERS = {
    "query_desc_default": ("QueryDesc", {"refined": "use_refined_sdf"}),
    "register_desc_default": ("RegisterDesc", {"refined": "use_refined_sdf"}),
    "register_volume_desc_default": ("RegisterVolumeDesc", {}),
    "fusion_mesh_desc_default": ("FusionMeshDesc", {}),
    "track_desc_default": ("TrackDesc", {"refined": "use_refined_sdf", "intr": "intrinsics4", "dist": "distortion5"}),
    "track_sdf_desc_default": ("TrackSdfDesc", {"refined": "use_refined_sdf", "intr": "intrinsics4", "dist": "distortion5"}),
    "track_rgbd_desc_default": ("TrackRgbdDesc", "track_desc_default"),
    "track_sdf_rgbd_desc_default": ("TrackSdfRgbdDesc", "track_sdf_desc_default"),
}
INTR, DIST = [501.0, 502.0, 303.0, 204.0], [0.01, -0.02, 0.03, 0.004, -0.005]


def _c_default(binding, L, name):
    d = getattr(binding, DESC_BUILDERS[name][0])()
    getattr(L, "i3d_" + name)(d)
    return d


@pytest.mark.parametrize("name", sorted(DESC_BUILDERS))
def test_descriptor_builders(name):
    """Every *_desc_default: the C default with no arguments, every alias in its field, and the differences between the builders that are easy to lose."""
    import ctypes
    binding, L = _lib()
    build = getattr(binding, name)
    struct, aliases = DESC_BUILDERS[name]
    ref = _c_default(binding, L, name)
    d = build()
    assert type(d) is getattr(binding, struct) and bytes(d) == bytes(ref)
    rgbd = isinstance(aliases, str)
    base_name = aliases if rgbd else name
    base_aliases = DESC_BUILDERS[base_name][1]
    inner = (lambda x: x.base) if rgbd else (lambda x: x)
    # aliases: the value lands in the field and nothing else moves (but use_context_camera, below)
    flipped = int(not inner(ref).use_refined_sdf) if "refined" in base_aliases else None
    for alias, field in base_aliases.items():
        for key in (alias, field):
            value = {"use_refined_sdf": flipped, "intrinsics4": INTR, "distortion5": DIST}[field]
            got = inner(build(**{key: value}))
            want = inner(_c_default(binding, L, name))
            setattr(want, field, value if field == "use_refined_sdf" else (ctypes.c_double * len(value))(*value))
            if base_name == "track_desc_default" and field != "use_refined_sdf":
                want.use_context_camera = 0
            assert bytes(got) == bytes(want), (key, field)
    if "refined" in base_aliases:
        assert inner(build(refined=True)).use_refined_sdf == 1 and inner(build(refined=0)).use_refined_sdf == 0 and inner(build(refined="x")).use_refined_sdf == 1
    else:
        with pytest.raises(ValueError) as e:
            build(refined=True)
        assert str(e.value) == f"{name}: unknown field refined"
    # intr / dist switch i3d_track_desc to its own camera and leave i3d_track_sdf_desc alone, in both directions
    if base_name == "track_desc_default":
        assert inner(build(use_context_camera=1)).use_context_camera == 1
        assert inner(build(use_context_camera=1, intr=INTR)).use_context_camera == 0 and inner(build(use_context_camera=1, dist=DIST)).use_context_camera == 0
        assert inner(build(intr=INTR, use_context_camera=1)).use_context_camera == 1
        assert list(inner(build(iterations=[3, 2])).iterations) == [3, 2, 0, 0] and list(inner(build(iterations=(7,))).iterations) == [7, 0, 0, 0]
        assert list(inner(build(iterations=[1, 2, 3, 4, 5])).iterations) == [1, 2, 3, 4]
    if base_name == "track_sdf_desc_default":
        assert inner(build(use_context_camera=1, intr=INTR, dist=DIST)).use_context_camera == 1
        assert inner(build(use_context_camera=0, intr=INTR, dist=DIST)).use_context_camera == 0
        assert inner(build(iterations=7)).iterations == 7
    if rgbd:
        d = build(photo_weight=2, geometric_weight=3, max_photo_residual=1)
        assert (d.geometric_weight, d.photo_weight, d.max_photo_residual) == (3.0, 2.0, 1.0) and bytes(d.base) == bytes(ref.base)
        assert build(photo_weight="0.25").photo_weight == 0.25          # float(): what ctypes alone refuses
        d = build(photo_weight=2, stop_rotation=1e-3)
        assert d.photo_weight == 2.0 and d.base.stop_rotation == 1e-3 and d.geometric_weight == ref.geometric_weight
        for own in ("base", "pad"):                                      # neither is a keyword: both go to the base builder, which has no such field
            with pytest.raises(ValueError) as e:
                build(**{own: 0})
            assert str(e.value) == f"{base_name}: unknown field {own}"
    # plain fields by their own names
    plain = {"query_desc_default": dict(project=0, max_steps=3, tolerance_voxels=0.5), "register_desc_default": dict(iterations=4, max_distance=0.25),
             "register_volume_desc_default": dict(iterations=5, stride=2, source_band_voxels=1.5), "fusion_mesh_desc_default": dict(min_weight=0.5, largest_component_only=1),
             "track_desc_default": dict(levels=2, max_distance=0.5, min_normal_dot=0.25, stop_translation=1e-3),
             "track_sdf_desc_default": dict(stride=2, huber_delta=0.125, max_depth=4.0, stop_rotation=1e-3)}[base_name]
    got = inner(build(**plain))
    assert all(getattr(got, k) == v for k, v in plain.items())
    with pytest.raises(ValueError) as e:
        build(bogus=1)
    assert str(e.value) == f"{base_name}: unknown field bogus"


TRACK_STATS = {"iterations": [1, 2, 3, 4], "status": 5, "valid_pixels": 6, "inliers": 7, "rms_initial": 8.5, "rms_final": 9.5, "min_pivot_ratio": 10.5}
TRACK_SDF_STATS = {"iterations": 1, "status": 2, "valid_pixels": 3, "valid": 4, "inliers": 5, "rms_initial": 6.5, "rms_final": 7.5, "min_pivot_ratio": 8.5}
PHOTO_STATS = {"photo_samples": 21, "photo_rms_initial": 22.5, "photo_rms_final": 23.5}
REGISTER_STATS = {"iterations": 1, "status": 2, "valid": 3, "inliers": 4, "rms_initial": 5.5, "rms_final": 6.5, "min_pivot_ratio": 7.5}
STATS_DICTS = {
    "TrackStats": TRACK_STATS,
    "TrackRgbdStats": {**TRACK_STATS, **PHOTO_STATS},
    "QueryStats": {"valid": 1, "projected": 2, "sum_abs_sdf": 3.5, "sum_sq_sdf": 4.5, "max_abs_sdf": 5.5, "sum_abs_distance": 6.5, "sum_sq_distance": 7.5,
                   "max_abs_distance": 8.5, "steps": 9},
    "RegisterStats": REGISTER_STATS,
    "RegisterVolumeStats": {**REGISTER_STATS, "selected": 8},
    "FusionMeshStats": {"stored": 1, "valid_cells": 2, "surface_cells": 3, "raw_triangles": 4, "vertices": 5, "corner_vertices": 6, "faces": 7, "degenerate_removed": 8,
                        "rounded_corner_occurrences": 9},
    "TrackSdfStats": TRACK_SDF_STATS,
    "TrackSdfRgbdStats": {**TRACK_SDF_STATS, **PHOTO_STATS},
}


@pytest.mark.parametrize("name", sorted(STATS_DICTS))
def test_stats_as_dict(name):
    """as_dict of every stats struct against a literal: the keys in order (a nested base first), float / int / list per key."""
    from intrinsic3d_amd import binding
    want = STATS_DICTS[name]
    st = getattr(binding, name)()
    for k, v in want.items():
        target = st.base if hasattr(st, "base") and k not in PHOTO_STATS else st
        if isinstance(v, list):
            getattr(target, k)[:] = v
        else:
            setattr(target, k, v)
    got = st.as_dict()
    assert got == want and list(got) == list(want)
    assert [type(v) for v in got.values()] == [type(v) for v in want.values()]
    assert all(type(x) is int for v in got.values() if isinstance(v, list) for x in v)


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
