"""The C ABI of libintrinsic3d_hip.so (include/intrinsic3d_hip.h) as data: the ctypes mirror of every struct and one prototype per function, both in the
header's order.  Nothing here loads the library: binding.load() walks PROTOTYPES, and tests/test_capi_surface.py holds both halves to the header - every
struct's size and field offsets through a C program, every prototype's parameter count and kinds through the header's text.

A new entry point is one line in PROTOTYPES (and a mirror with its _c_name_ when it brings a struct); the tests fail until the line agrees with the header.
"""
from __future__ import annotations

import ctypes as C

vp, cp, P = C.c_void_p, C.c_char_p, C.POINTER
i32, u32, i64, u64, f32, f64 = C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_float, C.c_double


class Stats(C.Structure):
    """The stats structs a method hands back as a dict."""

    def as_dict(self):
        """{field: float | int | list}, the fields of a nested `base` first"""
        d = {}
        for k, t in self._fields_:
            v = getattr(self, k)
            if k == "base":
                d.update(v.as_dict())
            else:
                d[k] = list(v) if issubclass(t, C.Array) else float(v) if t in (f32, f64) else int(v)
        return d


# ---- the structs, in the header's order -------------------------------------------------------------------------------------------------
class GridView(C.Structure):
    _c_name_ = "i3d_grid_view"
    _fields_ = [("num_voxels", i64), ("voxel_size", f32), ("truncation", f32),
                ("keys", vp), ("sdf", vp), ("sdf_refined", vp), ("albedo", vp),
                ("weight", vp), ("color", vp)]


class OptimizerConfig(C.Structure):
    """Optimizer::Config (optimizer.h:67-84) + the Intrinsic3D::Config / Optimizer::Data fields the path reads."""
    _c_name_ = "i3d_optimizer_config"
    _fields_ = [("iterations", i32), ("lm_steps", i32),
                ("lambda_g", f64), ("lambda_r0", f64), ("lambda_r1", f64),
                ("lambda_s0", f64), ("lambda_s1", f64), ("lambda_a", f64),
                ("fix_poses", i32), ("fix_intrinsics", i32), ("fix_distortion", i32),
                ("occlusion_distance", f32), ("num_observations", i32),
                ("thres_shell", f64), ("grid_level", i32), ("rgbd_level", i32),
                ("pcg_fixed_iterations", i32), ("verbose", i32), ("carry_trust_radius", i32), ("fix_sdf", i32)]


class IterationStats(C.Structure):
    _c_name_ = "i3d_iteration_stats"
    _fields_ = [("rows", i64 * 4), ("weight_sum", f64 * 4), ("type_weight", f64 * 4),
                ("valid_voxels", i64), ("free_parameters", i64),
                ("cost_initial", f64), ("cost_final", f64),
                ("lm_iterations", i32), ("successful_steps", i32), ("termination", i32),
                ("pcg_iterations", i32 * 50), ("step_accepted", i32 * 50), ("num_attempts", i32),
                ("final_radius", f64), ("time_add", f64), ("time_build", f64), ("time_solve", f64)]


class ShStats(C.Structure):
    _c_name_ = "i3d_sh_stats"
    _fields_ = [("data_rows", i64), ("reg_rows", i64), ("subvolumes", i32), ("lm_iterations", i32),
                ("termination", i32), ("cost_initial", f64), ("cost_final", f64)]


class RefineConfig(C.Structure):
    _c_name_ = "i3d_refine_config"
    _fields_ = [("num_grid_levels", i32), ("num_rgbd_levels", i32),
                ("thin_shell_factor", f64), ("thin_shell_factor_final", f64),
                ("clear_distant_voxels", i32), ("occlusion_distance", f32), ("num_observations", i32),
                ("subvolume_size_sh", f32), ("sh_lambda_reg", f64)]


REFINE_CALLBACK = C.CFUNCTYPE(None, vp, i32, i32, i32, i32)      # i3d_refine_callback


class RenderDesc(C.Structure):
    _c_name_ = "i3d_render_desc"
    _fields_ = [("frame", i32), ("level", i32), ("use_refined_sdf", i32), ("width", i32), ("height", i32),
                ("intrinsics4", f64 * 4), ("distortion5", f64 * 5), ("pose6", f64 * 6),
                ("min_depth", f32), ("max_depth", f32)]


class RenderStats(Stats):
    _c_name_ = "i3d_render_stats"
    _fields_ = [("hits", i64), ("samples", i64), ("residual_sq_sum", f64)]


class TrackDesc(C.Structure):
    _c_name_ = "i3d_track_desc"
    _fields_ = [("levels", i32), ("iterations", i32 * 4), ("use_refined_sdf", i32), ("use_context_camera", i32),
                ("intrinsics4", f64 * 4), ("distortion5", f64 * 5),
                ("max_distance", f32), ("min_normal_dot", f32), ("min_depth", f32), ("max_depth", f32),
                ("stop_rotation", f64), ("stop_translation", f64)]


class TrackStats(Stats):
    _c_name_ = "i3d_track_stats"
    _fields_ = [("iterations", i32 * 4), ("status", i32), ("valid_pixels", i64), ("inliers", i64),
                ("rms_initial", f64), ("rms_final", f64), ("min_pivot_ratio", f64)]


class TrackRgbdDesc(C.Structure):
    _c_name_ = "i3d_track_rgbd_desc"
    _fields_ = [("base", TrackDesc), ("geometric_weight", f64), ("photo_weight", f64), ("max_photo_residual", f32), ("pad", i32)]


class TrackRgbdStats(Stats):
    _c_name_ = "i3d_track_rgbd_stats"
    _fields_ = [("base", TrackStats), ("photo_samples", i64), ("photo_rms_initial", f64), ("photo_rms_final", f64)]


class MergeStats(C.Structure):
    """Not a Stats: Fusion.merge hands the motion back as numpy arrays and leaves `pad` out."""
    _c_name_ = "i3d_merge_stats"
    _fields_ = [("ordinal", u64), ("source_voxels", i64), ("sampled", i64), ("allocated", i64), ("aligned", i32), ("pad", i32),
                ("rotation", f64 * 9), ("translation_voxels", f64 * 3)]


class QueryDesc(C.Structure):
    _c_name_ = "i3d_query_desc"
    _fields_ = [("use_refined_sdf", i32), ("project", i32), ("max_steps", i32), ("tolerance_voxels", f64)]


class QueryStats(Stats):
    _c_name_ = "i3d_query_stats"
    _fields_ = [("valid", i64), ("projected", i64), ("sum_abs_sdf", f64), ("sum_sq_sdf", f64), ("max_abs_sdf", f64),
                ("sum_abs_distance", f64), ("sum_sq_distance", f64), ("max_abs_distance", f64), ("steps", i64)]


class RegisterDesc(C.Structure):
    _c_name_ = "i3d_register_desc"
    _fields_ = [("use_refined_sdf", i32), ("iterations", i32), ("max_distance", f64), ("stop_rotation", f64),
                ("stop_translation", f64)]


class RegisterStats(Stats):
    _c_name_ = "i3d_register_stats"
    _fields_ = [("iterations", i32), ("status", i32), ("valid", i64), ("inliers", i64), ("rms_initial", f64),
                ("rms_final", f64), ("min_pivot_ratio", f64)]


class RegisterVolumeDesc(C.Structure):
    _c_name_ = "i3d_register_volume_desc"
    _fields_ = [("iterations", i32), ("stride", i32), ("source_band_voxels", f64), ("max_distance", f64), ("stop_rotation", f64),
                ("stop_translation", f64)]


class RegisterVolumeStats(Stats):
    _c_name_ = "i3d_register_volume_stats"
    _fields_ = RegisterStats._fields_ + [("selected", i64)]


class FusionMeshDesc(C.Structure):
    _c_name_ = "i3d_fusion_mesh_desc"
    _fields_ = [("min_weight", f32), ("largest_component_only", i32)]


class FusionMeshStats(Stats):
    _c_name_ = "i3d_fusion_mesh_stats"
    _fields_ = [(k, i64) for k in ("stored", "valid_cells", "surface_cells", "raw_triangles", "vertices", "corner_vertices", "faces", "degenerate_removed",
                                   "rounded_corner_occurrences")]


class TrackSdfDesc(C.Structure):
    _c_name_ = "i3d_track_sdf_desc"
    _fields_ = [("use_refined_sdf", i32), ("use_context_camera", i32), ("intrinsics4", f64 * 4), ("distortion5", f64 * 5),
                ("iterations", i32), ("stride", i32), ("max_distance", f64), ("huber_delta", f64),
                ("min_depth", f32), ("max_depth", f32), ("stop_rotation", f64), ("stop_translation", f64)]


class TrackSdfStats(Stats):
    _c_name_ = "i3d_track_sdf_stats"
    _fields_ = [("iterations", i32), ("status", i32), ("valid_pixels", i64), ("valid", i64), ("inliers", i64),
                ("rms_initial", f64), ("rms_final", f64), ("min_pivot_ratio", f64)]


class TrackSdfRgbdDesc(C.Structure):
    _c_name_ = "i3d_track_sdf_rgbd_desc"
    _fields_ = [("base", TrackSdfDesc), ("geometric_weight", f64), ("photo_weight", f64), ("max_photo_residual", f32), ("pad", i32)]


class TrackSdfRgbdStats(Stats):
    _c_name_ = "i3d_track_sdf_rgbd_stats"
    _fields_ = [("base", TrackSdfStats), ("photo_samples", i64), ("photo_rms_initial", f64), ("photo_rms_final", f64)]


class LmScriptDesc(C.Structure):
    _c_name_ = "i3d_lm_script_desc"
    _fields_ = [("cost", f64), ("ngrad", f64), ("nfree", f64), ("radius0", f64), ("lm_steps", i32),
                ("K", i32), ("fix_poses", i32), ("fix_intr", i32), ("fix_dist", i32), ("n_attempts", i32), ("n_plan", i32), ("max_setups", i32),
                ("cdiag", vp), ("tri", vp), ("tail_c", vp), ("tail_S", vp),
                ("xbr", vp), ("d2xx", vp), ("pcg_it", vp), ("pcg_done", vp), ("norms2", vp), ("cand_cost", vp), ("debug_invalid", vp),
                ("plan", vp)]


# ---- the functions, in the header's order: (name, restype, argtypes) ---------------------------------------------------------------------
# A handle or an array the caller owns is vp, a path cp; P(..) where a method passes C.byref of a struct or of one scalar.
PROTOTYPES = [
    ("i3d_create", i32, [i32, P(vp)]),
    ("i3d_destroy", None, [vp]),
    ("i3d_last_error", cp, [vp]),
    ("i3d_version", cp, []),
    ("i3d_set_grid", i32, [vp, P(GridView)]),
    ("i3d_get_grid", i32, [vp, vp, vp]),
    ("i3d_update_grid", i32, [vp, vp, vp, vp]),
    ("i3d_set_frames", i32, [vp, i32, i32, vp, vp, vp, vp, vp]),
    ("i3d_set_camera", i32, [vp, vp, vp, vp]),
    ("i3d_get_camera", i32, [vp, vp, vp, vp]),
    ("i3d_set_voxel_sh", i32, [vp, vp]),
    ("i3d_get_voxel_sh", i32, [vp, vp]),
    ("i3d_set_frames_rgbd", i32, [vp, i32, i32, i32, i32, vp, vp]),
    ("i3d_get_frame_image", i32, [vp, i32, i32, vp, vp]),
    ("i3d_resize_depth", i32, [i32, i32, i32, vp, vp, i32, i32, vp, vp]),
    ("i3d_optimizer_config_default", None, [P(OptimizerConfig)]),
    ("i3d_optimize", i32, [vp, P(OptimizerConfig), vp]),
    ("i3d_optimize_host", i32, [i32, P(OptimizerConfig), P(GridView), vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    ("i3d_estimate_sh", i32, [vp, f32, f64, f64, P(i32), vp, vp, i32, P(ShStats)]),
    ("i3d_set_grid_from_tsdf_records", i32, [vp, f32, i64, vp, vp, vp, vp]),
    ("i3d_recompute_colors", i32, [vp, f32, i32]),
    ("i3d_clear_outside_thin_shell", i32, [vp, f64, P(i64)]),
    ("i3d_upsample", i32, [vp, P(i64)]),
    ("i3d_grid_info", i32, [vp, P(i64), P(f32), P(f32)]),
    ("i3d_export_grid", i32, [vp, vp, vp, vp, vp, vp, vp]),
    ("i3d_refine", i32, [vp, P(RefineConfig), P(OptimizerConfig), REFINE_CALLBACK, vp]),
    ("i3d_tsdf_read_header", i32, [cp, P(f32), P(f32), P(f32), P(u64), P(f32)]),
    ("i3d_tsdf_read_records", i32, [cp, u64, vp, vp, vp, vp]),
    ("i3d_tsdf_write", i32, [cp, f32, f32, f32, f32, u64, vp, vp, vp, vp]),
    ("i3d_sbr_write", i32, [cp, f32, f32, f32, f32, u64, vp, vp, vp, vp, vp, vp]),
    ("i3d_sbr_read", i32, [cp, u64, vp, vp, vp, vp, vp, vp]),
    ("i3d_write_poses", i32, [cp, i32, vp, vp]),
    ("i3d_write_intrinsics", i32, [cp, i32, i32, vp, vp]),
    ("i3d_read_intrinsics", i32, [cp, P(i32), P(i32), vp, vp]),
    ("i3d_config_load_yaml", i32, [cp, P(RefineConfig), P(OptimizerConfig)]),
    ("i3d_yaml_get", i32, [cp, cp, vp, u64]),
    ("i3d_extract_mesh", i32, [vp, i32, i32, i32, P(i64), P(i64)]),
    ("i3d_get_mesh", i32, [vp, vp, vp, vp]),
    ("i3d_export_mesh_ply", i32, [vp, cp, i32, i32, i32]),
    ("i3d_write_ply", i32, [cp, i64, vp, vp, i64, vp]),
    ("i3d_mesh_remove_loose_components", i32, [vp, vp, vp, vp, vp]),
    ("i3d_visualization_colors", i32, [i32, f32, i64, vp, vp, vp, vp, vp, vp, f32, i32, vp, vp, vp]),
    ("i3d_mc_tables", i32, [vp, vp]),
    ("i3d_render_view", i32, [vp, P(RenderDesc), vp, vp, vp, vp, vp, vp, P(RenderStats)]),
    ("i3d_track_desc_default", None, [P(TrackDesc)]),
    ("i3d_track_frame", i32, [vp, P(TrackDesc), i32, i32, vp, vp, P(TrackStats)]),
    ("i3d_debug_track_sums", i32, [vp, P(TrackDesc), i32, i32, vp, i32, vp, vp, vp, vp]),
    ("i3d_track_rgbd_desc_default", None, [P(TrackRgbdDesc)]),
    ("i3d_track_frame_rgbd", i32, [vp, P(TrackRgbdDesc), i32, i32, vp, vp, vp, P(TrackRgbdStats)]),
    ("i3d_debug_track_rgbd_sums", i32, [vp, P(TrackRgbdDesc), i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
    ("i3d_png_info", i32, [vp, u64, vp, vp, vp, vp]),
    ("i3d_png_decode", i32, [vp, u64, vp, u64]),
    ("i3d_pose_mat_to_vec6", i32, [vp, vp]),
    ("i3d_sensor_open", i32, [cp, i32, f32, f32, P(vp)]),
    ("i3d_sensor_open_yaml", i32, [cp, P(vp), P(f32), P(f32)]),
    ("i3d_sensor_close", None, [vp]),
    ("i3d_sensor_info", i32, [vp, vp, vp, vp, vp, vp, vp]),
    ("i3d_sensor_color", i32, [vp, i32, vp]),
    ("i3d_sensor_depth", i32, [vp, i32, vp]),
    ("i3d_sensor_pose", i32, [vp, i32, vp]),
    ("i3d_sensor_set_pose", i32, [vp, i32, vp]),
    ("i3d_sensor_set_pose_vec6", i32, [vp, i32, vp]),
    ("i3d_sensor_save_poses", i32, [vp, cp]),
    ("i3d_keyframes_load", i32, [cp, vp, u64, vp, vp, vp]),
    ("i3d_keyframes_save", i32, [cp, i32, u64, vp, vp]),
    ("i3d_keyframes_select", i32, [i32, u64, vp, vp]),
    ("i3d_blur_score", i32, [vp, i32, i32, i32, vp]),
    ("i3d_init_frames_from_sensor", i32, [vp, i32, vp, u64, vp, i32, i32, vp, vp]),
    ("i3d_fusion_create", i32, [i32, f32, f32, f32, vp, u64, P(vp)]),
    ("i3d_fusion_destroy", None, [vp]),
    ("i3d_fusion_last_error", cp, [vp]),
    ("i3d_fusion_integrate", i32, [vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, i32]),
    ("i3d_fusion_finish", i32, [vp, i32, vp]),
    ("i3d_fusion_info", i32, [vp, vp, vp, vp, vp]),
    ("i3d_fusion_get", i32, [vp, vp, vp, vp, vp]),
    ("i3d_fusion_save", i32, [vp, cp]),
    ("i3d_fusion_insert_records", i32, [vp, u64, vp, vp, vp, vp]),
    ("i3d_fusion_load", i32, [i32, cp, f32, f32, vp, P(vp)]),
    ("i3d_fusion_snapshot", i32, [vp, P(u64)]),
    ("i3d_fusion_deintegrate", i32, [vp, u64, i32, i32, vp, i32, i32, vp, vp, vp, vp, i32]),
    ("i3d_fusion_reintegrate", i32, [vp, u64, i32, i32, vp, i32, i32, vp, vp, vp, vp, i32, vp, P(u64)]),
    ("i3d_fusion_merge", i32, [vp, vp, vp, P(MergeStats)]),
    ("i3d_fusion_prune", i32, [vp, f32, f32, i32, vp, i32, vp]),
    ("i3d_fusion_components", i32, [vp, f32, f32, vp]),
    ("i3d_fusion_get_components", i32, [vp, vp, vp, vp]),
    ("i3d_fusion_prune_components", i32, [vp, f32, f32, i64, i64, i32, vp]),
    ("i3d_fusion_render", i32, [vp, P(RenderDesc), vp, vp, P(RenderStats)]),
    ("i3d_fusion_track", i32, [vp, P(TrackDesc), i32, i32, vp, vp, P(TrackStats)]),
    ("i3d_query_desc_default", None, [P(QueryDesc)]),
    ("i3d_query_points", i32, [vp, P(QueryDesc), i64, vp, vp, vp, vp, vp, vp, vp, P(QueryStats)]),
    ("i3d_fusion_query_points", i32, [vp, P(QueryDesc), i64, vp, vp, vp, vp, vp, vp, P(QueryStats)]),
    ("i3d_cast_rays", i32, [vp, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, P(RenderStats)]),
    ("i3d_fusion_cast_rays", i32, [vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, P(RenderStats)]),
    ("i3d_render_view_color", i32, [vp, P(RenderDesc), vp, vp, P(RenderStats)]),
    ("i3d_fusion_render_color", i32, [vp, P(RenderDesc), vp, vp, P(RenderStats)]),
    ("i3d_cast_rays_color", i32, [vp, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, P(RenderStats)]),
    ("i3d_fusion_cast_rays_color", i32, [vp, i32, i64, vp, vp, vp, vp, vp, vp, vp, P(RenderStats)]),
    ("i3d_register_desc_default", None, [P(RegisterDesc)]),
    ("i3d_register_points", i32, [vp, P(RegisterDesc), i64, vp, vp, P(RegisterStats)]),
    ("i3d_fusion_register_points", i32, [vp, P(RegisterDesc), i64, vp, vp, P(RegisterStats)]),
    ("i3d_register_volume_desc_default", None, [P(RegisterVolumeDesc)]),
    ("i3d_fusion_register_volume", i32, [vp, vp, P(RegisterVolumeDesc), vp, P(RegisterVolumeStats)]),
    ("i3d_fusion_mesh_desc_default", None, [P(FusionMeshDesc)]),
    ("i3d_fusion_extract_mesh", i32, [vp, P(FusionMeshDesc), P(i64), P(i64), P(FusionMeshStats)]),
    ("i3d_fusion_get_mesh", i32, [vp, vp, vp, vp]),
    ("i3d_fusion_export_mesh_ply", i32, [vp, P(FusionMeshDesc), cp]),
    ("i3d_track_sdf_desc_default", None, [P(TrackSdfDesc)]),
    ("i3d_track_frame_sdf", i32, [vp, P(TrackSdfDesc), i32, i32, vp, vp, P(TrackSdfStats)]),
    ("i3d_fusion_track_sdf", i32, [vp, P(TrackSdfDesc), i32, i32, vp, vp, P(TrackSdfStats)]),
    ("i3d_track_frames_sdf", i32, [vp, P(TrackSdfDesc), i32, i32, i32, vp, vp, vp]),
    ("i3d_track_keyframes_sdf", i32, [vp, P(TrackSdfDesc), i32, i32, vp, vp, vp]),
    ("i3d_track_sdf_rgbd_desc_default", None, [P(TrackSdfRgbdDesc)]),
    ("i3d_track_frame_sdf_rgbd", i32, [vp, P(TrackSdfRgbdDesc), i32, i32, vp, vp, vp, P(TrackSdfRgbdStats)]),
    ("i3d_fusion_track_sdf_rgbd", i32, [vp, P(TrackSdfRgbdDesc), i32, i32, vp, vp, vp, P(TrackSdfRgbdStats)]),
    ("i3d_track_frames_sdf_rgbd", i32, [vp, P(TrackSdfRgbdDesc), i32, i32, i32, vp, vp, vp, vp]),
    ("i3d_track_keyframes_sdf_rgbd", i32, [vp, P(TrackSdfRgbdDesc), i32, i32, vp, vp, vp]),
    ("i3d_comm_unique_id", i32, [vp, P(i32)]),
    ("i3d_comm_init", i32, [vp, i32, i32, vp, i32]),
    ("i3d_comm_sim_create", vp, [i32]),
    ("i3d_comm_sim_destroy", None, [vp]),
    ("i3d_comm_init_sim", i32, [vp, vp, i32]),
    ("i3d_shard_plan", i32, [i32, i32, i32, vp, vp, P(i32), P(i32), P(i32), vp]),
    ("i3d_shard_vec_index", i32, [i32, i32, i32]),
    ("i3d_shard_need", i32, [i32, i32, vp, vp, vp]),
    ("i3d_comm_stats", i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    ("i3d_comm_transport", cp, [vp]),
    ("i3d_timing_enable", i32, [vp, i32]),
    ("i3d_timing_select", i32, [vp, u32]),
    ("i3d_timing_get", i32, [vp, vp, vp, i32]),
    ("i3d_timing_get_work", i32, [vp, vp, vp]),
    ("i3d_timing_get_work_ex", i32, [vp, vp, vp, vp, vp]),
    ("i3d_kernel_name", cp, [i32]),
    ("i3d_problem_sizes", i32, [vp, vp]),
    ("i3d_debug_assemble", i32, [vp, P(OptimizerConfig), i32, P(i32)]),
    ("i3d_debug_map_order", i64, [vp, i64, i32, vp]),
    ("i3d_debug_flags", i32, [vp, vp]),
    ("i3d_debug_eg_rows", i32, [vp, vp, vp, vp, vp]),
    ("i3d_debug_reg_rows", i32, [vp, vp, vp, vp]),
    ("i3d_debug_neighbors", i32, [vp, vp]),
    ("i3d_debug_normal_eq", i32, [vp, vp, vp, P(f64)]),
    ("i3d_debug_jtj_apply", i32, [vp, vp, vp]),
    ("i3d_debug_work_list", i32, [vp, vp, i64, P(i64)]),
    ("i3d_debug_counters", i32, [vp, vp]),
    ("i3d_debug_ladder_stats", i32, [vp, vp]),
    ("i3d_debug_ladder_passes", i32, [vp, vp]),
    ("i3d_debug_lm_script", i32, [vp, P(LmScriptDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    ("i3d_debug_cull_stats", i32, [vp, vp, vp]),
    ("i3d_debug_register_sums", i32, [vp, P(RegisterDesc), i64, vp, vp, vp, vp, P(i64)]),
    ("i3d_debug_register_row_cap", i32, [vp, i32]),
    ("i3d_debug_track_sdf_sums", i32, [vp, P(TrackSdfDesc), i32, i32, vp, vp, vp, vp, P(i64), P(i64)]),
    ("i3d_debug_track_batch_frames", i32, [vp, i32]),
    ("i3d_debug_track_sdf_rgbd_sums", i32, [vp, P(TrackSdfRgbdDesc), i32, i32, vp, vp, vp, vp, vp, P(i64), P(i64)]),
    ("i3d_debug_voxel_intensity", i32, [vp, i32, vp]),
    ("i3d_debug_sh_stages", i32, [vp, f32, f64, i32, P(i32), vp, vp, vp, vp]),
    ("i3d_fusion_debug_voxel_luminance", i32, [vp, i64, vp, vp]),
    ("i3d_fusion_debug_track_sdf_rgbd_sums", i32, [vp, P(TrackSdfRgbdDesc), i32, i32, vp, vp, vp, vp, vp, P(i64), P(i64)]),
    ("i3d_fusion_debug_voxels", i32, [vp, i64, vp, vp, vp, vp, vp, vp]),
    ("i3d_fusion_debug_frame_samples", i32, [vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, i32, i64, vp, vp, vp, vp, vp, vp]),
    ("i3d_fusion_debug_poke_voxels", i32, [vp, i64, vp, vp, vp, vp, vp]),
    ("i3d_fusion_debug_register_volume_selection", i32, [vp, P(RegisterVolumeDesc), i64, vp, vp, P(i64)]),
    ("i3d_fusion_debug_register_volume_sums", i32, [vp, vp, P(RegisterVolumeDesc), vp, vp, i64, i32, vp, P(i64), P(i64)]),
    ("i3d_fusion_debug_insertion_order", i32, [vp, u64, vp, P(u64)]),
]

EXPORTS = [name for name, _, _ in PROTOTYPES]
