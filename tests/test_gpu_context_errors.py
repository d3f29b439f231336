"""The fault table of the context layer (grid in and out, keyframes and camera, level transitions, the parity probes of the assembled solver state, the
lighting entry points' validation), pinned completely: for every call that validation must refuse, the return code, the whole text of i3d_last_error, and
that no output was written.  The expected values are tests/golden/context_errors.json, recorded once
(`python tests/test_gpu_context_errors.py --record [path]`) with the library as it stood before the context host was consolidated (one visit-order record, one
order crossing, one entry guard); they never come from the code under test.

Some entry points answer a refused call with a bare code and leave the error text alone, others write a text; on a null handle the text is the
thread's create error.  So every case starts from a known text: `i3d_optimize(handle, NULL, NULL)` on a handle, `i3d_create(0, NULL)` on the null
handle.  A case whose recorded text is that primer's is one that writes none.

Handles: the null handle; an empty context; a 3 x 3 x 3 grid; the same with 8 x 6 one-level keyframes (no colour); the same with a camera; the same with
colour keyframes; the same after i3d_debug_assemble (the one case whose set-up launches kernels: a work-list capacity can only be too small for a work list)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fault_table import Outs, compare_with_golden, record_golden  # noqa: E402
from intrinsic3d_amd import binding as B  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "context_errors.json")
p = B._p
N, VS, W, H, K = 27, 0.01, 8, 6, 2
F64, I32, U8, F32 = np.float64, np.int32, np.uint8, np.float32


def small_grid():
    """3 x 3 x 3 voxels around the origin, the surface through the middle layer"""
    keys = np.stack(np.meshgrid(np.arange(-1, 2), np.arange(-1, 2), np.arange(-1, 2), indexing="ij"), -1).reshape(-1, 3).astype(I32)
    sdf = keys[:, 2].astype(F64) * VS
    return dict(keys=keys, sdf=sdf, sdf_refined=sdf.copy(), albedo=np.full(N, 0.6), weight=np.ones(N, F32), color=np.full((N, 3), 128, U8))


GRID = small_grid()


def grid_view(n=N, **none):
    a = {k: (None if k in none else p(v)) for k, v in GRID.items()}
    return B.GridView(n, VS, 5 * VS, a["keys"], a["sdf"], a["sdf_refined"], a["albedo"], a["weight"], a["color"])


def frames(color):
    f = dict(lum=[np.full((H, W), 0.5, F32)], depth=[np.ones((H, W), F32)])
    if color:
        f["bgr"] = [np.full((H, W, 3), 100, U8)]
    return [dict(f) for _ in range(K)]


SIZES = (np.array([W], I32), np.array([H], I32))
IMG = np.zeros((H, W), F32)
BGR = np.zeros((H, W, 3), U8)
PTRS = (C.c_void_p * K)(*[IMG.ctypes.data] * K)
BGR_PTRS = (C.c_void_p * K)(*[BGR.ctypes.data] * K)
CAMERA = (np.array([30.0, 30.0, 3.5, 2.5]), np.zeros(5), np.zeros((K, 6)))
RECORDS = (GRID["keys"], GRID["sdf"].astype(F32), GRID["weight"], GRID["color"])
UID = np.zeros(128, U8)


def _grid_cases(L):
    """set_grid, get_grid, update_grid, export_grid, grid_info, set_grid_from_tsdf_records, the voxel-SH pair"""
    set_grid = lambda gv: (lambda h, o: L.i3d_set_grid(h, C.byref(gv) if gv is not None else None))
    get_grid = lambda h, o: L.i3d_get_grid(h, p(o.arr(N, F64)), p(o.arr(N, F64)))
    update = lambda h, o: L.i3d_update_grid(h, p(GRID["sdf"]), p(GRID["albedo"]), p(GRID["color"]))
    export = lambda h, o: L.i3d_export_grid(h, p(o.arr((N, 3), I32)), p(o.arr(N, F64)), p(o.arr(N, F64)), p(o.arr(N, F64)), p(o.arr(N, F32)), p(o.arr((N, 3), U8)))
    info = lambda h, o: L.i3d_grid_info(h, o.i64(), C.cast(p(o.arr(1, F32)), C.POINTER(C.c_float)), C.cast(p(o.arr(1, F32)), C.POINTER(C.c_float)))
    records = lambda n=N, keys=RECORDS[0], sdf=RECORDS[1]: (lambda h, o: L.i3d_set_grid_from_tsdf_records(h, VS, n, p(keys), p(sdf), p(RECORDS[2]), p(RECORDS[3])))
    set_sh = lambda sh: (lambda h, o: L.i3d_set_voxel_sh(h, p(sh)))
    get_sh = lambda out: (lambda h, o: L.i3d_get_voxel_sh(h, p(o.arr((N, 9), F64)) if out else None))
    sh = np.zeros((N, 9))
    return [("set_grid/null_handle", "null", set_grid(grid_view())), ("set_grid/null_view", "empty", set_grid(None)),
            ("set_grid/empty", "empty", set_grid(grid_view(0))), ("set_grid/negative_count", "empty", set_grid(grid_view(-1))),
            ("set_grid/null_keys", "empty", set_grid(grid_view(keys=1))), ("set_grid/null_sdf", "empty", set_grid(grid_view(sdf=1))),
            ("set_grid/null_sdf_refined", "empty", set_grid(grid_view(sdf_refined=1))), ("set_grid/null_albedo", "empty", set_grid(grid_view(albedo=1))),
            ("set_grid/null_weight", "empty", set_grid(grid_view(weight=1))), ("set_grid/null_color", "grid", set_grid(grid_view(color=1))),
            ("set_grid/more_than_2^30", "empty", set_grid(grid_view((1 << 30) + 1))), ("set_grid/more_than_2^30_on_a_grid", "grid", set_grid(grid_view((1 << 30) + 1))),
            ("set_grid/null_keys_before_2^30", "empty", set_grid(grid_view((1 << 30) + 1, keys=1))),
            ("get_grid/null_handle", "null", get_grid), ("get_grid/no_grid", "empty", get_grid),
            ("update_grid/null_handle", "null", update), ("update_grid/no_grid", "empty", update),
            ("export_grid/null_handle", "null", export), ("export_grid/no_grid", "empty", export),
            ("grid_info/null_handle", "null", info), ("grid_info/no_grid", "empty", info),
            ("set_grid_from_tsdf_records/null_handle", "null", records()), ("set_grid_from_tsdf_records/n_0", "empty", records(0)),
            ("set_grid_from_tsdf_records/n_negative", "grid", records(-1)), ("set_grid_from_tsdf_records/null_keys", "empty", records(keys=None)),
            ("set_grid_from_tsdf_records/null_sdf", "grid", records(sdf=None)),
            ("set_voxel_sh/null_handle", "null", set_sh(sh)), ("set_voxel_sh/null_pointer", "grid", set_sh(None)), ("set_voxel_sh/no_grid", "empty", set_sh(sh)),
            ("set_voxel_sh/null_pointer_before_no_grid", "empty", set_sh(None)),
            ("get_voxel_sh/null_handle", "null", get_sh(True)), ("get_voxel_sh/null_pointer", "grid", get_sh(False)), ("get_voxel_sh/no_grid", "empty", get_sh(True))]


def _frame_cases(L):
    """both set_frames, get_frame_image, the camera pair"""
    def set_frames(k=K, levels=1, ws=SIZES[0], hs=SIZES[1], lum=PTRS, dep=PTRS):
        return lambda h, o: L.i3d_set_frames(h, k, levels, p(ws), p(hs), C.cast(lum, C.c_void_p) if lum else None, C.cast(dep, C.c_void_p) if dep else None, None)

    def rgbd(k=K, levels=1, w=W, h_=H, bgr=BGR_PTRS, dep=PTRS):
        return lambda h, o: L.i3d_set_frames_rgbd(h, k, levels, w, h_, C.cast(bgr, C.c_void_p) if bgr else None, C.cast(dep, C.c_void_p) if dep else None)
    image = lambda frame, level: (lambda h, o: L.i3d_get_frame_image(h, frame, level, p(o.arr((H, W), F32)), p(o.arr((H, W), F32))))
    set_cam = lambda i=0, d=1, q=2: (lambda h, o: L.i3d_set_camera(h, *[None if j is None else p(CAMERA[j]) for j in (i, d, q)]))
    get_cam = lambda h, o: L.i3d_get_camera(h, p(o.arr(4, F64)), p(o.arr(5, F64)), p(o.arr((K, 6), F64)))
    return [("set_frames/null_handle", "null", set_frames()), ("set_frames/K_0", "grid", set_frames(k=0)), ("set_frames/levels_0", "grid", set_frames(levels=0)),
            ("set_frames/null_widths", "grid", set_frames(ws=None)), ("set_frames/null_heights", "empty", set_frames(hs=None)),
            ("set_frames/null_lum", "grid", set_frames(lum=None)), ("set_frames/null_depth", "keyed", set_frames(dep=None)),
            ("set_frames_rgbd/null_handle", "null", rgbd()), ("set_frames_rgbd/K_0", "grid", rgbd(k=0)), ("set_frames_rgbd/levels_negative", "grid", rgbd(levels=-1)),
            ("set_frames_rgbd/width_0", "empty", rgbd(w=0)), ("set_frames_rgbd/height_0", "grid", rgbd(h_=0)), ("set_frames_rgbd/null_bgr", "grid", rgbd(bgr=None)),
            ("set_frames_rgbd/null_depth", "keyed", rgbd(dep=None)),
            ("set_frames_rgbd/4_levels_of_8x6", "grid", rgbd(levels=4)), ("set_frames_rgbd/5_levels_of_8x6", "keyed", rgbd(levels=5)),
            ("set_frames_rgbd/null_bgr_before_levels", "grid", rgbd(levels=4, bgr=None)),
            ("get_frame_image/null_handle", "null", image(0, 0)), ("get_frame_image/no_frames", "grid", image(0, 0)), ("get_frame_image/frame_2", "framed", image(K, 0)),
            ("get_frame_image/frame_negative", "keyed", image(-1, 0)), ("get_frame_image/level_1", "framed", image(0, 1)), ("get_frame_image/level_negative", "keyed", image(1, -1)),
            ("set_camera/null_handle", "null", set_cam()), ("set_camera/null_intrinsics", "framed", set_cam(i=None)), ("set_camera/null_distortion", "framed", set_cam(d=None)),
            ("set_camera/null_poses", "keyed", set_cam(q=None)), ("set_camera/frames_first", "grid", set_cam()), ("set_camera/frames_first_on_an_empty_context", "empty", set_cam()),
            ("set_camera/null_pointer_before_frames_first", "grid", set_cam(q=None)),
            ("get_camera/null_handle", "null", get_cam), ("get_camera/no_camera", "framed", get_cam), ("get_camera/nothing_set", "empty", get_cam)]


def _level_cases(L):
    """recompute_colors, clear_outside_thin_shell, upsample, refine, the lighting entry points"""
    recolor = lambda nobs=5: (lambda h, o: L.i3d_recompute_colors(h, 0.02, nobs))
    clear = lambda h, o: L.i3d_clear_outside_thin_shell(h, 2 * VS, o.i64())
    up = lambda h, o: L.i3d_upsample(h, o.i64())
    ocfg = B.default_config(iterations=1, thres_shell=2 * VS)
    rcfg = lambda **kw: B.RefineConfig(**dict(dict(num_grid_levels=1, num_rgbd_levels=1, thin_shell_factor=2.0, thin_shell_factor_final=1.0, clear_distant_voxels=1,
                                                   occlusion_distance=0.02, num_observations=5, subvolume_size_sh=0.05, sh_lambda_reg=10.0), **kw))
    refine = lambda rc, oc=ocfg: (lambda h, o: L.i3d_refine(h, C.byref(rc) if rc is not None else None, C.byref(oc) if oc is not None else None, B.REFINE_CALLBACK(), None))

    def estimate(thres):
        return lambda h, o: L.i3d_estimate_sh(h, 0.05, 10.0, thres, C.cast(p(o.arr(1, I32)), C.POINTER(C.c_int32)), p(o.arr((4, 9), F64)), p(o.arr((4, 3), I32)), 4, o.stats(B.ShStats))

    def stages(thres):
        return lambda h, o: L.i3d_debug_sh_stages(h, 0.05, thres, 4, C.cast(p(o.arr(1, I32)), C.POINTER(C.c_int32)), p(o.arr((4, 3), I32)), p(o.arr((4, 100), F64)),
                                                  p(o.arr(4, F64)), p(o.arr(N, I32)))
    return [("recompute_colors/null_handle", "null", recolor()), ("recompute_colors/nothing_set", "empty", recolor()), ("recompute_colors/no_frames", "grid", recolor()),
            ("recompute_colors/no_camera", "framed", recolor()), ("recompute_colors/no_colour_images", "keyed", recolor()),
            ("recompute_colors/no_colour_images_before_9_observations", "keyed", recolor(9)), ("recompute_colors/9_observations", "colored", recolor(9)),
            ("clear_outside_thin_shell/null_handle", "null", clear), ("clear_outside_thin_shell/no_grid", "empty", clear),
            ("upsample/null_handle", "null", up), ("upsample/no_grid", "empty", up),
            ("refine/null_handle", "null", refine(rcfg())), ("refine/null_refine_config", "grid", refine(None)), ("refine/null_optimizer_config", "grid", refine(rcfg(), None)),
            ("refine/no_grid", "empty", refine(rcfg())), ("refine/0_grid_levels", "keyed", refine(rcfg(num_grid_levels=0))),
            ("refine/0_rgbd_levels", "keyed", refine(rcfg(num_rgbd_levels=0))), ("refine/2_rgbd_levels_of_1", "keyed", refine(rcfg(num_rgbd_levels=2))),
            ("refine/1_rgbd_level_of_0", "grid", refine(rcfg())), ("refine/no_camera", "framed", refine(rcfg())), ("refine/no_colour_images", "keyed", refine(rcfg())),
            ("refine/9_observations", "colored", refine(rcfg(num_observations=9))),
            ("estimate_sh/null_handle", "null", estimate(2 * VS)), ("estimate_sh/no_grid", "empty", estimate(2 * VS)), ("estimate_sh/thres_shell_0", "grid", estimate(0.0)),
            ("estimate_sh/thres_shell_nan", "keyed", estimate(float("nan"))), ("estimate_sh/no_grid_before_thres_shell", "empty", estimate(-1.0)),
            ("debug_sh_stages/null_handle", "null", stages(2 * VS)), ("debug_sh_stages/no_grid", "empty", stages(2 * VS)), ("debug_sh_stages/thres_shell_0", "grid", stages(0.0))]


def _probe_cases(L):
    """optimize's and the communicator's argument checks, and the readbacks of assembled solver state before and after i3d_debug_assemble"""
    cfg = B.default_config(iterations=1, thres_shell=2 * VS)
    NP = 2 * N + 6 * K + 9
    x = np.zeros(NP)
    optimize = lambda h, o: L.i3d_optimize(h, None, None)
    assemble = lambda c: (lambda h, o: L.i3d_debug_assemble(h, C.byref(c) if c is not None else None, 0, C.cast(p(o.arr(1, I32)), C.POINTER(C.c_int32))))
    flags = lambda out=True: (lambda h, o: L.i3d_debug_flags(h, p(o.arr(N, U8)) if out else None))
    nbrs = lambda out=True: (lambda h, o: L.i3d_debug_neighbors(h, p(o.arr((N, 18), I32)) if out else None))
    eg = lambda h, o: L.i3d_debug_eg_rows(h, p(o.arr((N, 8), I32)), p(o.arr((N, 8), F32)), p(o.arr((N, 8), F32)), None)
    reg = lambda h, o: L.i3d_debug_reg_rows(h, p(o.arr(N, U8)), p(o.arr(N, U8)), p(o.arr((N, 6), F32)))
    normal = lambda h, o: L.i3d_debug_normal_eq(h, p(o.arr(NP, F64)), p(o.arr(NP, F64)), C.cast(p(o.arr(1, F64)), C.POINTER(C.c_double)))
    jtj = lambda xin=x, out=True: (lambda h, o: L.i3d_debug_jtj_apply(h, p(xin), p(o.arr(NP, F64)) if out else None))
    work = lambda idx=True, cnt=True, cap=N: (lambda h, o: L.i3d_debug_work_list(h, p(o.arr(N, I32)) if idx else None, cap, o.i64() if cnt else None))

    def work_too_small(h, o):      # the work list of the assembled handle has A entries: a capacity of A - 1 (-1 for an empty list)
        n = C.c_int64(-1)
        assert L.i3d_debug_work_list(h, None, 0, C.byref(n)) == 0
        return L.i3d_debug_work_list(h, p(o.arr(N, I32)), n.value - 1, None)
    bare = lambda fn, *a: (lambda h, o: getattr(L, fn)(h, *a))
    cull = lambda a=True, b=True: (lambda h, o: L.i3d_debug_cull_stats(h, p(o.arr(1, np.int64)) if a else None, p(o.arr(1, np.int64)) if b else None))
    return [("optimize/null_handle", "null", optimize), ("optimize/null_config", "grid", optimize),
            ("debug_assemble/null_handle", "null", assemble(cfg)), ("debug_assemble/null_config", "keyed", assemble(None)),
            ("debug_flags/null_handle", "null", flags()), ("debug_flags/null_pointer", "grid", flags(False)), ("debug_flags/no_grid", "empty", flags()),
            ("debug_neighbors/null_handle", "null", nbrs()), ("debug_neighbors/null_pointer", "grid", nbrs(False)), ("debug_neighbors/no_grid", "empty", nbrs()),
            ("debug_eg_rows/null_handle", "null", eg), ("debug_eg_rows/nothing_set", "empty", eg), ("debug_eg_rows/not_assembled", "keyed", eg),
            ("debug_reg_rows/null_handle", "null", reg), ("debug_reg_rows/no_frames", "grid", reg), ("debug_reg_rows/not_assembled", "keyed", reg),
            ("debug_normal_eq/null_handle", "null", normal), ("debug_normal_eq/nothing_set", "empty", normal), ("debug_normal_eq/not_assembled", "keyed", normal),
            ("debug_jtj_apply/null_handle", "null", jtj()), ("debug_jtj_apply/null_x", "keyed", jtj(None)), ("debug_jtj_apply/null_y", "keyed", jtj(out=False)),
            ("debug_jtj_apply/not_assembled", "keyed", jtj()), ("debug_jtj_apply/null_y_when_assembled", "assembled", jtj(out=False)),
            ("debug_work_list/null_handle", "null", work()), ("debug_work_list/null_pointers", "keyed", work(False, False)),
            ("debug_work_list/not_assembled", "keyed", work()), ("debug_work_list/count_alone_not_assembled", "grid", work(idx=False)),
            ("debug_work_list/null_pointers_when_assembled", "assembled", work(False, False)), ("debug_work_list/capacity_too_small", "assembled", work_too_small),
            ("debug_work_list/capacity_negative", "assembled", work(cnt=False, cap=-1)),
            ("debug_cull_stats/null_handle", "null", cull()), ("debug_cull_stats/null_pairs", "keyed", cull(a=False)), ("debug_cull_stats/null_culled", "keyed", cull(b=False)),
            ("debug_cull_stats/nothing_assembled", "keyed", cull()),
            ("problem_sizes/null_handle", "null", lambda h, o: L.i3d_problem_sizes(h, p(o.arr(6, np.int64)))), ("problem_sizes/null_pointer", "grid", bare("i3d_problem_sizes", None)),
            ("debug_counters/null_handle", "null", lambda h, o: L.i3d_debug_counters(h, p(o.arr(1, np.int64)))),
            ("debug_ladder_stats/null_handle", "null", lambda h, o: L.i3d_debug_ladder_stats(h, p(o.arr(6, np.int64)))),
            ("debug_ladder_stats/null_pointer", "grid", bare("i3d_debug_ladder_stats", None)),
            ("debug_ladder_passes/null_handle", "null", lambda h, o: L.i3d_debug_ladder_passes(h, p(o.arr(8, np.int64)))),
            ("debug_ladder_passes/null_pointer", "grid", bare("i3d_debug_ladder_passes", None)),
            ("comm_stats/null_handle", "null", lambda h, o: L.i3d_comm_stats(h, *[p(o.arr(1, np.int64)) for _ in range(4)], *[p(o.arr(1, I32)) for _ in range(4)])),
            ("comm_init/null_handle", "null", bare("i3d_comm_init", 0, 1, p(UID), 128)), ("comm_init/null_id", "grid", bare("i3d_comm_init", 0, 1, None, 128)),
            ("comm_init/world_0", "grid", bare("i3d_comm_init", 0, 0, p(UID), 128)), ("comm_init/rank_negative", "grid", bare("i3d_comm_init", -1, 2, p(UID), 128)),
            ("comm_init/rank_2_of_2", "empty", bare("i3d_comm_init", 2, 2, p(UID), 128)),
            ("comm_init_sim/null_handle", "null", bare("i3d_comm_init_sim", p(UID), 0)), ("comm_init_sim/null_shared", "grid", bare("i3d_comm_init_sim", None, 0)),
            ("timing_enable/null_handle", "null", bare("i3d_timing_enable", 1)), ("timing_select/null_handle", "null", bare("i3d_timing_select", 1)),
            ("timing_get/null_handle", "null", lambda h, o: L.i3d_timing_get(h, p(o.arr(12, F64)), p(o.arr(12, np.int64)), 0)),
            ("timing_get_work/null_handle", "null", lambda h, o: L.i3d_timing_get_work(h, p(o.arr(12, F64)), p(o.arr(12, np.int64)))),
            ("timing_get_work_ex/null_handle", "null", lambda h, o: L.i3d_timing_get_work_ex(h, p(o.arr(12, F64)), p(o.arr(12, np.int64)), p(o.arr(12, F64)), p(o.arr(12, np.int64))))]


def table(L):
    """every case: (name, stage of the handle it runs on, call(handle, outs) -> return code)"""
    cases = _grid_cases(L) + _frame_cases(L) + _level_cases(L) + _probe_cases(L)
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return cases


def run_table():
    """the table on its handles -> [{name, code, error, untouched}]; every handle must come out of its stage in the state it went in with"""
    L = B.load()
    cases = table(L)
    out = {}

    def stage(name, ctx):
        h = ctx.h if ctx is not None else None
        state = None if ctx is None else (ctx.export_grid() if name != "empty" else None)
        for case, _, call in (c for c in cases if c[1] == name):
            if h is None:
                assert L.i3d_create(0, None) != 0
            else:
                assert L.i3d_optimize(h, None, None) != 0
            o = Outs()
            rc = call(h, o)
            out[case] = dict(name=case, code=int(rc), error=L.i3d_last_error(h).decode(), untouched=bool(o.untouched()))
        if state is not None:      # a refused call changed no voxel either
            after = ctx.export_grid()
            assert all(np.array_equal(state[k], after[k]) for k in state), name

    stage("null", None)
    with B.Context(0) as empty:
        stage("empty", empty)
    with B.Context(0) as ctx:
        ctx.set_grid(VS, *[GRID[k] for k in ("keys", "sdf", "sdf_refined", "albedo", "weight", "color")])
        stage("grid", ctx)
        ctx.set_frames(frames(False), 1)
        stage("framed", ctx)
        ctx.set_camera(*CAMERA)
        stage("keyed", ctx)
        ctx.set_frames(frames(True), 1)
        stage("colored", ctx)
        ctx.debug_assemble(B.default_config(iterations=1, thres_shell=2 * VS), 0)
        stage("assembled", ctx)
    return [out[c[0]] for c in cases]


def test_fault_table_equals_the_recorded_one():
    compare_with_golden(GOLDEN, run_table())


if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] != "--record":
        sys.exit("usage: test_gpu_context_errors.py --record [path]   (writes the fault table of the loaded library)")
    sys.exit(record_golden(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, run_table(), B.LIB_PATH))
