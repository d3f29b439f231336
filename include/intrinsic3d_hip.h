/* intrinsic3d_hip.h — C ABI of the MI355X-native (gfx950, HIP) implementation of NVlabs/intrinsic3d's
 * voxel-SDF shading-optimisation hot path.
 *
 * The reference has no FFI layer; the boundary this library replaces is the C++ entry point
 *
 *     bool nv::Optimizer::optimize(SDFColorization&, Optimizer::Data&, Optimizer::ImageFormationModel&)
 *                                   libintrinsic3d/include/nv/refinement/optimizer.h:123-125
 *                                   libintrinsic3d/src/refinement/optimizer.cpp:109-173
 *
 * and its sibling  nv::LightingSVSH::estimate() + computeVoxelShCoeffs()
 *                                   libintrinsic3d/include/nv/lighting/lighting_svsh.h:52,60
 *                                   libintrinsic3d/src/lighting/lighting_svsh.cpp:93-110,166-346
 *
 * i.e. everything the reference hands to Ceres (nls_solver.cpp:190-367).  Plain pointers and sizes only; no
 * C++/torch types cross this boundary.  All functions return 0 on success and a non-zero i3d_status otherwise
 * (the reference's convention is bool + std::cerr, optimizer.cpp:113-114); nothing throws.  One host thread
 * drives a context.  INTEGRATION.md shows the reference-side shim that binds these entry points.
 */
#ifndef INTRINSIC3D_HIP_H
#define INTRINSIC3D_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct i3d_context i3d_context;

typedef enum {
    I3D_OK = 0,
    I3D_ERR_INVALID_ARGUMENT = 1,   /* null grid / iterations < 1 (optimizer.cpp:113-114 returns false) */
    I3D_ERR_NO_DEVICE = 2,          /* no HIP device: the product path never falls back to the CPU */
    I3D_ERR_HIP = 3,
    I3D_ERR_STATE = 4,              /* grid / frames / camera not set */
    I3D_ERR_CAPACITY = 5,
    I3D_ERR_COMM = 6,
    I3D_ERR_IO = 7                  /* file missing / truncated (SparseVoxelGrid::load, Camera::load return false) */
} i3d_status;

/* ---- lifetime ------------------------------------------------------------------------------------------ */
int  i3d_create(int32_t device_ordinal, i3d_context** out);
void i3d_destroy(i3d_context* ctx);
/* last error text of this context (ctx may be NULL for creation errors) */
const char* i3d_last_error(const i3d_context* ctx);
const char* i3d_version(void);

/* ---- voxel grid: SparseVoxelGrid<VoxelSBR> (sparse_voxel_grid.h:69-161) as flat arrays ---------------------
 * Arrays are in the caller's grid->begin()..end() iteration order.  That "visit order" is part of the
 * reference's result (the albedo-regulariser edge set depends on it, optimizer.cpp:264-279) and is kept as
 * a per-voxel rank on the device. */
typedef struct {
    int64_t        num_voxels;
    float          voxel_size;     /* SparseVoxelGrid::voxelSize() */
    float          truncation;     /* SparseVoxelGrid::truncation() = 5*voxel_size (sparse_voxel_grid.cpp:48) */
    const int32_t* keys;           /* [N][3] voxel coordinates */
    const double*  sdf;            /* VoxelSBR::sdf          (read-only for the path) */
    const double*  sdf_refined;    /* VoxelSBR::sdf_refined  (optimised in place)     */
    const double*  albedo;         /* VoxelSBR::albedo       (optimised in place)     */
    const float*   weight;         /* VoxelSBR::weight */
    const uint8_t* color;          /* [N][3] VoxelSBR::color (r,g,b) */
} i3d_grid_view;

int i3d_set_grid(i3d_context* ctx, const i3d_grid_view* grid);
/* write-back of the only per-voxel fields the path mutates; either pointer may be NULL */
int i3d_get_grid(i3d_context* ctx, double* sdf_refined, double* albedo);
/* overwrite the unknowns / colours of the resident grid (visit order); NULL = keep */
int i3d_update_grid(i3d_context* ctx, const double* sdf_refined, const double* albedo, const uint8_t* color);

/* ---- keyframes: ImageFormationModel::rgbd_pyr + ShadingCostData (optimizer.h:107-115, shading_cost.h:52-73)
 * lum/depth/bgr[f*levels + lvl]; float luminance in [0,1] (pyramid.cpp:66-74), float depth in metres (0 = invalid),
 * optional 8-bit BGR (only needed by i3d_recompute_colors).  Images are copied to the device. */
int i3d_set_frames(i3d_context* ctx, int32_t num_frames, int32_t levels, const int32_t* widths, const int32_t* heights,
                   const float* const* lum, const float* const* depth, const uint8_t* const* bgr);

/* ---- camera: intrinsics Vec4 (fx,fy,cx,cy at level 0), distortion Vec5 (k1,k2,k3,p1,p2), poses Vec6[K]
 * (angle-axis, translation; world->camera) — optimizer.h:109-114 */
int i3d_set_camera(i3d_context* ctx, const double* intrinsics4, const double* distortion5, const double* poses6k);
int i3d_get_camera(i3d_context* ctx, double* intrinsics4, double* distortion5, double* poses6k);

/* ---- Optimizer::Data::voxel_sh_coeffs (optimizer.h:96): 9 doubles per voxel, visit order ------------------ */
int i3d_set_voxel_sh(i3d_context* ctx, const double* voxel_sh);
int i3d_get_voxel_sh(i3d_context* ctx, double* voxel_sh);

/* Intrinsic3D::init's Pyramid(num_rgbd_levels, color, depth) per keyframe, built on the device from level-0 colour + depth (already in colour
 * geometry): float luminance (convertTo 1/255 + BGR2GRAY), cv::pyrDown levels, valid-mean depth levels (rgbd/pyramid.cpp:59-166).
 * Replaces i3d_set_frames for callers that do not want to build the pyramids with OpenCV. */
int i3d_set_frames_rgbd(i3d_context* ctx, int32_t num_frames, int32_t levels, int32_t width, int32_t height, const uint8_t* const* bgr, const float* const* depth);
int i3d_get_frame_image(i3d_context* ctx, int32_t frame, int32_t level, float* lum /* may be NULL */, float* depth /* may be NULL */);
/* resizeDepth (rgbd/processing.cpp:129-181): a depth image resampled into the colour camera's geometry; intrinsics = {fx, fy, cx, cy} */
int i3d_resize_depth(int32_t device_ordinal, int32_t in_w, int32_t in_h, const float* depth_in, const float* in_intr4, int32_t out_w, int32_t out_h,
                     const float* out_intr4, float* depth_out);

/* ---- Optimizer::Config (optimizer.h:67-84) + the fields of Intrinsic3D::Config / Optimizer::Data the path reads */
typedef struct {
    int32_t iterations;            /* outer Gauss-Newton iterations (optimizer.cpp:119) */
    int32_t lm_steps;              /* max LM attempts per iteration (nls_solver.cpp:300) */
    double  lambda_g, lambda_r0, lambda_r1, lambda_s0, lambda_s1, lambda_a;
    int32_t fix_poses, fix_intrinsics, fix_distortion;
    float   occlusion_distance;    /* SDFColorization::Config::max_occlusion_distance (intrinsic3d.cpp:165) */
    int32_t num_observations;      /* ...::max_num_observations (intrinsic3d.cpp:166) */
    double  thres_shell;           /* Optimizer::Data::thres_shell */
    int32_t grid_level, rgbd_level;
    /* parity / measurement controls (not in the reference) */
    int32_t pcg_fixed_iterations;  /* >=0: run exactly this many PCG iterations per LM attempt; -1: Ceres' Q-test */
    int32_t verbose;
    int32_t carry_trust_radius;    /* extension, default 0 = the reference's ACTUAL behaviour.  1: start every outer iteration at the trust-region radius the
                                      previous one ended with — what nls_solver.cpp:322-323 is written to do but never does (a fresh NLSSolver is
                                      constructed per iteration, optimizer.cpp:138, so solver_info_ is always empty).  Saves the ~5 rejected LM attempts
                                      that re-discover the radius every iteration; results then differ from the reference's. */
    int32_t fix_sdf;               /* extension: every sdf_refined block constant (BASELINE.json configs[0], "albedo-only"); the reference has
                                      no such switch — Optimizer::fixVoxelParams (optimizer.cpp:312-361) fixes per voxel only */
} i3d_optimizer_config;

void i3d_optimizer_config_default(i3d_optimizer_config* cfg);   /* the reference's struct defaults */

/* per outer iteration: the quantities NLSSolver prints (nls_solver.cpp:57-103) */
typedef struct {
    int64_t rows[4];               /* Eg, Er, Es, Ea residual blocks */
    double  weight_sum[4];         /* per-type sum of row weights before normalisation */
    double  type_weight[4];        /* lambda_t / weight_sum_t * 1000 (nls_solver.cpp:379-394) */
    int64_t valid_voxels;          /* "voxels (valid n)" of optimizer.cpp:158 */
    int64_t free_parameters;
    double  cost_initial, cost_final;
    int32_t lm_iterations, successful_steps, termination;   /* termination: 0 no-conv, 1 convergence, 2 first successful step, 3 failure */
    int32_t pcg_iterations[50];    /* one per LM attempt */
    int32_t step_accepted[50];
    int32_t num_attempts;
    double  final_radius;
    double  time_add, time_build, time_solve;               /* seconds, the reference's split (nls_solver.cpp:66-67,101) */
} i3d_iteration_stats;

/* Optimizer::optimize on the resident grid / frames / camera / per-voxel SH.  stats: [cfg->iterations] or NULL. */
int i3d_optimize(i3d_context* ctx, const i3d_optimizer_config* cfg, i3d_iteration_stats* stats);

/* One-shot drop-in with host buffers (upload, optimize, write back sdf_refined/albedo/camera in place). */
int i3d_optimize_host(int32_t device_ordinal, const i3d_optimizer_config* cfg, const i3d_grid_view* grid,
                      double* sdf_refined_io, double* albedo_io,
                      int32_t num_frames, int32_t levels, const int32_t* widths, const int32_t* heights,
                      const float* const* lum, const float* const* depth,
                      double* intrinsics4_io, double* distortion5_io, double* poses6k_io,
                      const double* voxel_sh, i3d_iteration_stats* stats);

/* ---- LightingSVSH(grid, subvolume_size, lambda_reg, thres_shell, weighted=true)::estimate() followed by
 * computeVoxelShCoeffs() (intrinsic3d.cpp:255-264).  sh: [cap][9], sub_index: [cap][3] or NULL.  The per-voxel
 * coefficients stay resident for i3d_optimize (fetch with i3d_get_voxel_sh). */
typedef struct { int64_t data_rows, reg_rows; int32_t subvolumes, lm_iterations, termination; double cost_initial, cost_final; } i3d_sh_stats;
int i3d_estimate_sh(i3d_context* ctx, float subvolume_size, double lambda_reg, double thres_shell,
                    int32_t* num_subvolumes, double* sh, int32_t* sub_index, int32_t cap, i3d_sh_stats* stats);

/* ---- level transitions and the refine schedule (Intrinsic3D::refine, intrinsic3d.cpp:206-409) ------------------------------
 * i3d_set_grid_from_tsdf_records: SparseVoxelGrid<Voxel>::load (records in file order) + SDFAlgorithms::convert (algorithms.cpp:47-72)
 * i3d_recompute_colors          : Intrinsic3D::recomputeColors (SDFColorization::add/compute, colorization.cpp:113-189,318-354)
 * i3d_clear_outside_thin_shell  : SDFAlgorithms::clearVoxelsOutsideThinShell (algorithms.cpp:368-458)
 * i3d_upsample                  : SDFAlgorithms::upsample (algorithms.cpp:202-235)
 * The grid stays resident; i3d_grid_info / i3d_export_grid return it in visit order (e.g. inside the refine callback). */
int i3d_set_grid_from_tsdf_records(i3d_context* ctx, float voxel_size, int64_t n, const int32_t* keys, const float* sdf, const float* weight, const uint8_t* color);
int i3d_recompute_colors(i3d_context* ctx, float occlusion_distance, int32_t num_observations);
int i3d_clear_outside_thin_shell(i3d_context* ctx, double thres_shell, int64_t* new_count);
int i3d_upsample(i3d_context* ctx, int64_t* new_count);
int i3d_grid_info(i3d_context* ctx, int64_t* num_voxels, float* voxel_size, float* truncation);
int i3d_export_grid(i3d_context* ctx, int32_t* keys, double* sdf, double* sdf_refined, double* albedo, float* weight, uint8_t* color);

typedef struct {                   /* Intrinsic3D::Config (intrinsic3d.h:67-84), keys of data/intrinsic3d.yml */
    int32_t num_grid_levels, num_rgbd_levels;
    double  thin_shell_factor, thin_shell_factor_final;
    int32_t clear_distant_voxels;
    float   occlusion_distance; int32_t num_observations;
    float   subvolume_size_sh; double sh_lambda_reg;
} i3d_refine_config;
/* RefinementCallback::onSDFRefined(RefinementInfo) (intrinsic3d.h:94-114) */
typedef void (*i3d_refine_callback)(void* user, int32_t grid_level, int32_t num_grid_levels, int32_t pyramid_level, int32_t num_pyramid_levels);
int i3d_refine(i3d_context* ctx, const i3d_refine_config* rcfg, const i3d_optimizer_config* ocfg, i3d_refine_callback cb, void* user);

/* ---- on-disk formats either side of the path (host-only; no device needed) -------------------------------------------------
 * .tsdf: header {f32 voxel_size, f32 truncation, f32 integration_weight_sample, u64 count, f32 max_load_factor} then count records
 *        {i32 x,y,z; f32 sdf; f32 weight; u8 r,g,b; u8 pad}  (SparseVoxelGrid<Voxel>::save/load, sparse_voxel_grid.cpp:484-569).
 * VoxelSBR dump: same header, records {i32 x,y,z; f64 sdf; f32 weight; u8 r,g,b,pad; f64 albedo; f64 sdf_refined} (44 bytes).
 * poses: TUM trajectory lines (Sensor::savePoses, rgbd/sensor.cpp:315-347); intrinsics: Camera::save/load (camera.cpp:202-274).
 * i3d_config_load_yaml reads the flat `key: "value"` map of data/intrinsic3d.yml into the two config structs. */
int i3d_tsdf_read_header(const char* path, float* voxel_size, float* truncation, float* integration_weight_sample, uint64_t* count, float* max_load_factor);
int i3d_tsdf_read_records(const char* path, uint64_t capacity, int32_t* keys, float* sdf, float* weight, uint8_t* color);
int i3d_tsdf_write(const char* path, float voxel_size, float truncation, float integration_weight_sample, float max_load_factor, uint64_t count,
                   const int32_t* keys, const float* sdf, const float* weight, const uint8_t* color);
int i3d_sbr_write(const char* path, float voxel_size, float truncation, float integration_weight_sample, float max_load_factor, uint64_t count,
                  const int32_t* keys, const double* sdf, const double* sdf_refined, const double* albedo, const float* weight, const uint8_t* color);
int i3d_sbr_read(const char* path, uint64_t capacity, int32_t* keys, double* sdf, double* sdf_refined, double* albedo, float* weight, uint8_t* color);
int i3d_write_poses(const char* path, int32_t num_frames, const double* timestamps, const double* poses_world_to_cam /* [K][6] */);
int i3d_write_intrinsics(const char* path, int32_t width, int32_t height, const double* intr4, const double* dist5);
int i3d_read_intrinsics(const char* path, int32_t* width, int32_t* height, double* intr4, double* dist5);
int i3d_config_load_yaml(const char* path, i3d_refine_config* rcfg, i3d_optimizer_config* ocfg);
int i3d_yaml_get(const char* path, const char* key, char* value, uint64_t capacity);     /* Settings::get<std::string>: any key of a flat yml */

/* ---- mesh export of the resident grid (MarchingCubes<VoxelSBR>::extractSurface, MeshUtil, Mesh::save; SDFVisualization::exportMesh) -----
 * use_refined_sdf: SDFAlgorithms::applyRefinedSdf before extraction (app_intrinsic3d.cpp:170-172).  color_mode: I3D_COLOR_* below — what
 * SDFVisualization::colorize paints on the voxels before the mesh of a mode is extracted (visualization.cpp:101-164, 228-373); the shading modes need the
 * lighting estimate of i3d_estimate_sh / i3d_refine.  largest_component_only: MeshUtil::removeLooseComponents.  PLY: binary_little_endian, float xyz, uchar rgb,
 * "uchar int" face lists (mesh.cpp:41-100). */
enum {
    I3D_COLOR_VOXEL = 0,                 /* ""                 the voxel colours */
    I3D_COLOR_ALBEDO = 1,                /* "albedo"           output_mesh_albedo            applyColorAlbedo            :308-315 */
    I3D_COLOR_NORMALS = 2,               /* "normals"          output_mesh_normals           applyColorNormals           :228-240 */
    I3D_COLOR_LAPLACIAN = 3,             /* "lap"              output_mesh_laplacian         applyColorLaplacian         :243-259 */
    I3D_COLOR_INTENSITY = 4,             /* "lum"              output_mesh_intensity         applyColorIntensity         :262-270 */
    I3D_COLOR_INTENSITY_GRAD = 5,        /* "lum_grad"         output_mesh_intensity_grad    applyColorIntensityGradient :273-305 */
    I3D_COLOR_SHADING = 6,               /* "shading_sv"       output_mesh_shading_sv        applyColorShading(false)    :318-359 */
    I3D_COLOR_SHADING_CONST_ALBEDO = 7,  /* "shading_sv_const" output_mesh_shading_sv_const  applyColorShading(true) */
    I3D_COLOR_CHROMACITY = 8             /* "chroma"           output_mesh_chromacity        applyColorChromacity        :362-373 */
    /* "subvol" / "subvol_interp" paint Subvolumes::color(), drawn from rand() in the reference (subvolumes.cpp:87-91): nothing to reproduce, not offered */
};
int i3d_extract_mesh(i3d_context* ctx, int32_t use_refined_sdf, int32_t color_mode, int32_t largest_component_only, int64_t* num_vertices, int64_t* num_faces);
int i3d_get_mesh(i3d_context* ctx, float* vertices /*[nv][3]*/, uint8_t* colors /*[nv][3]*/, int32_t* faces /*[nf][3]*/);
int i3d_export_mesh_ply(i3d_context* ctx, const char* path, int32_t use_refined_sdf, int32_t color_mode, int32_t largest_component_only);
int i3d_write_ply(const char* path, int64_t num_vertices, const float* vertices, const uint8_t* colors /* may be NULL */, int64_t num_faces, const int32_t* faces);
/* MeshUtil::removeLooseComponents + removeUnusedVertices (mesh/util.cpp:47-171) on caller arrays, in place (what largest_component_only applies): keeps the
 * largest connected component (first one among equals, components numbered by their first face), drops the vertices no face uses; counts updated.  Host only. */
int i3d_mesh_remove_loose_components(int64_t* num_vertices, float* vertices, uint8_t* colors /* may be NULL */, int64_t* num_faces, int32_t* faces);
/* SDFVisualization::applyColor* on caller arrays (voxels in any order; subvolumes as i3d_estimate_sh returns them, only read by the shading modes): the colour
 * every voxel gets in a colour mode.  The same function the export kernel runs, instantiated for the host.  visit_rank: the position of every voxel in the
 * reference's walk over its grid (NULL: the array order) — "lum_grad" is painted in place there, a voxel reads its +x neighbour repainted if the walk passed
 * it earlier (visualization.cpp:273-305), and the export reproduces that from the resident grid's visit order.  Host only. */
int i3d_visualization_colors(int32_t color_mode, float voxel_size, int64_t num_voxels, const int32_t* keys, const double* sdf_refined, const double* albedo, const float* weight,
                             const uint8_t* color, const int64_t* visit_rank /* or NULL */, float subvolume_size, int32_t num_subvolumes, const int32_t* subvolume_index /* [S][3] or NULL */,
                             const double* subvolume_sh /* [S][9] or NULL */, uint8_t* color_out /* [n][3] */);
int i3d_mc_tables(uint8_t* ntri /*[256]*/, int8_t* tri /*[256][16]*/);      /* the triangulation table (Bourke's, as in marching_cubes.cpp:330-623); returns max triangles per cell */

/* ---- image-space view of the resident model: ray casting of the SDF into one camera (DESIGN.md section 13 defines every output) -----------
 * Cells as the marching cubes sees them (all 8 corners stored with weight != 0), trilinear field, secant-refined zero crossing from outside.  Reads the grid, the
 * per-voxel SH, the camera and the keyframe luminance; changes nothing the optimiser reads (the brick bitmap of the empty-space skipping is cached in the context
 * and dropped whenever the set of stored voxels changes). */
typedef struct {
    int32_t frame;            /* >= 0: keyframe of the context: its refined pose, the refined intrinsics at `level`, residual available.
                                 -1: the camera given below */
    int32_t level;            /* pyramid level (frame >= 0): image size of that level, intrinsics x 2^-level */
    int32_t use_refined_sdf;  /* 1: sdf_refined (the optimiser's unknowns), 0: the fused sdf (as i3d_extract_mesh) */
    int32_t width, height;    /* frame < 0 only */
    double intrinsics4[4], distortion5[5], pose6[6];   /* frame < 0 only; pose world->camera, angle-axis | t, as i3d_set_camera */
    float min_depth, max_depth;                        /* camera-z range of the march; <= 0: unbounded on that side */
} i3d_render_desc;

typedef struct { int64_t hits; int64_t samples; double residual_sq_sum; } i3d_render_stats;

/* Ray-casts the resident grid into one view.  Every output is [h][w] (normal: [h][w][3]); any may be NULL; stats may be NULL.
 * depth = camera z of the hit (0 = no hit), normal = unit SDF gradient in the world frame, albedo, shading = SH(normal) with the per-voxel SH, intensity =
 * albedo * shading, residual = intensity - keyframe luminance (frame >= 0 only).  residual_sq_sum is summed when the residual plane is requested. */
int i3d_render_view(i3d_context* ctx, const i3d_render_desc* desc, float* depth, float* normal, float* albedo,
                    float* shading, float* intensity, float* residual, i3d_render_stats* stats);

/* ---- registration of a depth frame against the resident model: projective point-to-plane ICP (DESIGN.md section 14 defines it) -------------
 * The model side is the ray cast of i3d_render_view (depth + world normal) at the level's starting pose; association, fp64 fixed-order sums and the 6-DoF
 * Gauss-Newton solve run on the device.  Needs a grid; the context's camera only with use_context_camera = 1; never keyframes or per-voxel SH.
 * Writes only buffers of its own: tracking changes nothing the optimiser reads. */
typedef struct {
    int32_t levels;              /* pyramid levels used, 1..4; coarse (levels-1) to fine (0) */
    int32_t iterations[4];       /* max Gauss-Newton iterations at level l, 0..100 (0: the level is skipped) */
    int32_t use_refined_sdf;     /* 1: sdf_refined, 0: the fused sdf (as i3d_render_view) */
    int32_t use_context_camera;  /* 1: the context's (refined) intrinsics + distortion; 0: the two fields below */
    double  intrinsics4[4], distortion5[5];            /* level 0, colour geometry */
    float   max_distance;        /* association gate |p - m|, metres (> 0) */
    float   min_normal_dot;      /* gate on n_model . n_frame (both world frame) */
    float   min_depth, max_depth;/* frame pixels outside are ignored; <= 0: open */
    double  stop_rotation, stop_translation;           /* a level ends when |omega| and |upsilon| of the step are both below */
} i3d_track_desc;

typedef struct {
    int32_t iterations[4];       /* iterations run per level */
    int32_t status;              /* 0 converged, 1 iteration limit, 2 too few inliers (pose unchanged), 3 degenerate system (pose left at the last good estimate) */
    int64_t valid_pixels, inliers;                     /* finest level, at the returned pose */
    double  rms_initial, rms_final;                    /* point-to-plane RMS over the inliers, metres, finest level: first association / at the returned pose */
    double  min_pivot_ratio;     /* min / max Cholesky pivot of the last 6x6 system: how well the geometry pins all six DoF.  With status 3 the factorisation
                                    stopped at the first pivot d that failed d > 1e-12 * trace: max(d, 0) / (the largest pivot up to and including that column
                                    if it is > 0, else the ratio is 0); always finite and in [0, 1] */
} i3d_track_stats;

void i3d_track_desc_default(i3d_track_desc* d);
/* depth: [height][width] metres in colour geometry, 0 = invalid.  pose6_io: world->camera, angle-axis | t, as i3d_set_camera; the initial guess in, the
 * registered pose out.  stats may be NULL. */
int  i3d_track_frame(i3d_context* ctx, const i3d_track_desc* desc, int32_t width, int32_t height, const float* depth, double* pose6_io, i3d_track_stats* stats);
/* debug entry, same family as i3d_debug_*: the 29 sums (21 upper-triangle J^T J row by row, 6 J^T r, r^2, count) and the inlier count of ONE association
 * pass at `level`: frame depth against the model ray-cast at pose_ref, frame points placed with pose_cur */
int  i3d_debug_track_sums(i3d_context* ctx, const i3d_track_desc* desc, int32_t width, int32_t height, const float* depth,
                          int32_t level, const double* pose_ref6, const double* pose_cur6, double* sums29, int64_t* inliers);

/* ---- registration by depth and model intensity (DESIGN.md section 16 defines it): i3d_track_frame with one more residual per pixel, the frame's luminance
 * against the model's predicted intensity (albedo x SH shading, the `intensity` plane of i3d_render_view) at the pixel's projection into the pass's ray cast.
 * J^T J = geometric_weight^2 sum J_g J_g^T + photo_weight^2 sum J_p J_p^T; photo_weight has the unit metres per unit luminance.  With photo_weight > 0 the
 * model needs its per-voxel SH (I3D_ERR_STATE without).  With geometric_weight = 1, photo_weight = 0 the result is i3d_track_frame's bit for bit.  Further
 * I3D_ERR_INVALID_ARGUMENT: a null luminance, a negative or non-finite weight, both weights 0.  Status 2 counts geometric inliers when geometric_weight > 0,
 * else photometric samples. */
typedef struct {
    i3d_track_desc base;
    double geometric_weight, photo_weight;             /* defaults 1 and 0.1 */
    float  max_photo_residual;                         /* gate on |I_model - I_frame|; <= 0 (default): open */
    int32_t pad;
} i3d_track_rgbd_desc;

typedef struct {
    i3d_track_stats base;
    int64_t photo_samples;                             /* finest level, at the returned pose */
    double  photo_rms_initial, photo_rms_final;        /* luminance RMS over the photometric samples: first association of level 0 / at the returned pose */
} i3d_track_rgbd_stats;

void i3d_track_rgbd_desc_default(i3d_track_rgbd_desc* d);
/* luminance: [height][width] float, the keyframes' convention (0.299 R + 0.587 G + 0.114 B over 255), colour geometry like the depth */
int  i3d_track_frame_rgbd(i3d_context* ctx, const i3d_track_rgbd_desc* desc, int32_t width, int32_t height, const float* depth, const float* luminance,
                          double* pose6_io, i3d_track_rgbd_stats* stats);
/* i3d_debug_track_sums of the combined system: the 27 weighted entries, geometric r^2 and count, then photometric r^2 and sample count */
int  i3d_debug_track_rgbd_sums(i3d_context* ctx, const i3d_track_rgbd_desc* desc, int32_t width, int32_t height, const float* depth, const float* luminance,
                               int32_t level, const double* pose_ref6, const double* pose_cur6, double* sums31, int64_t* inliers, int64_t* photo_samples);

/* ---- dataset loader in front of the path.  Host code except i3d_init_frames_from_sensor.
 * PNG: the layout cv::imdecode(IMREAD_UNCHANGED) returns — interleaved, B,G,R[,A] order, 8-bit or native-endian 16-bit, palette and
 * 1/2/4-bit images expanded (rgbd/sensor_i3d.cpp:307-327). */
int i3d_png_info(const uint8_t* data, uint64_t size, int32_t* width, int32_t* height, int32_t* channels, int32_t* bit_depth);
int i3d_png_decode(const uint8_t* data, uint64_t size, void* pixels, uint64_t capacity_bytes);
/* Intrinsic3D::init's pose conversion (intrinsic3d.cpp:189-192): camera-to-world Mat4f (row-major) -> world-to-camera Vec6 (angle-axis, t) */
int i3d_pose_mat_to_vec6(const float* cam_to_world16, double* pose6);
/* Sensor::create + SensorI3d::init (sensor.cpp:63-96, sensor_i3d.cpp:60-144): `frame-%06d.{color,depth}.png`, `.pose.txt`,
 * `{depth,color}Intrinsics.txt` of `folder`; max_frames / min_depth / max_depth as in sensor.yml (0 = off) */
typedef struct i3d_sensor i3d_sensor;
int  i3d_sensor_open(const char* folder, int32_t max_frames, float min_depth, float max_depth, i3d_sensor** out);
/* Sensor::create(Settings&) (rgbd/sensor.cpp:64-118) over a sensor.yml: keys dataset, max_frames, min_depth, max_depth, converted like Settings::get<T> (settings.cpp:86-109);
 * the depth range read from the file is handed back (AppFusion sizes its volume with it, app_fusion.cpp:131-133). */
int  i3d_sensor_open_yaml(const char* sensor_yml, i3d_sensor** out, float* min_depth /* may be NULL */, float* max_depth /* may be NULL */);
void i3d_sensor_close(i3d_sensor* s);
int  i3d_sensor_info(const i3d_sensor* s, int32_t* num_frames, int32_t* num_loaded, int32_t* color_wh /*[2]*/, int32_t* depth_wh /*[2]*/,
                     float* color_intr4 /* fx fy cx cy */, float* depth_intr4);
int  i3d_sensor_color(const i3d_sensor* s, int32_t id, uint8_t* bgr /*[h][w][3]*/);          /* Sensor::color */
int  i3d_sensor_depth(const i3d_sensor* s, int32_t id, float* depth /*[h][w] metres*/);      /* Sensor::depth: decode, 1/1000, thresholdDepth */
int  i3d_sensor_pose(const i3d_sensor* s, int32_t id, float* cam_to_world16);
int  i3d_sensor_set_pose(i3d_sensor* s, int32_t id, const float* cam_to_world16);
int  i3d_sensor_set_pose_vec6(i3d_sensor* s, int32_t id, const double* pose_world_to_cam6);  /* finishRgbdLevel write-back, intrinsic3d.cpp:362-368 */
int  i3d_sensor_save_poses(const i3d_sensor* s, const char* path);                           /* Sensor::savePoses, sensor.cpp:315-347 */
/* KeyframeSelection::load / save / selectKeyframes (keyframe_selection.cpp:73-106,139-207); count = lines in the file even if > capacity */
int i3d_keyframes_load(const char* path, int32_t* window_size, uint64_t capacity, double* scores, uint8_t* is_keyframe, uint64_t* count);
int i3d_keyframes_save(const char* path, int32_t window_size, uint64_t count, const double* scores, const uint8_t* is_keyframe);
int i3d_keyframes_select(int32_t window_size, uint64_t count, const double* scores, uint8_t* is_keyframe);
/* KeyframeSelection::estimateBlur (keyframe_selection.cpp:219-311): blur metric of one colour (B,G,R) or grey 8-bit image; 1 = sharp */
int i3d_blur_score(const uint8_t* image, int32_t width, int32_t height, int32_t channels, double* score);
/* Intrinsic3D::init's keyframe loop (intrinsic3d.cpp:156-193): for every keyframe decode colour + depth, resample the depth into the colour
 * geometry and build the pyramids on the device, convert the pose; sets the frames and the camera (colour intrinsics, zero distortion) of ctx */
int i3d_init_frames_from_sensor(i3d_context* ctx, int32_t device_ordinal, const i3d_sensor* s, uint64_t num_flags, const uint8_t* is_keyframe,
                                int32_t num_rgbd_levels, int32_t frame_capacity, int32_t* frame_ids, int32_t* num_keyframes);

/* ---- TSDF fusion, the stage in front of the path: AppFusion::fuseSDF's volume on the device.
 * i3d_fusion_create    SparseVoxelGrid<Voxel>::create(voxel_size, depth_min, depth_max) + setClipBounds (app_fusion.cpp:121-139); clip6 = {x0,x1,y0,y1,z0,z1},
 *                      all zero / NULL = no clipping; initial_capacity = expected number of allocated voxels (the table grows when needed)
 * i3d_fusion_integrate erodeDiscontinuities(depth, erode_window) + computeNormals + SparseVoxelGrid::integrate (alloc + update) of one frame
 *                      (app_fusion.cpp:152-166, sparse_voxel_grid.cpp:301-467); depth = Sensor::depth (metres, 0 = invalid), pose = camera-to-world
 * i3d_fusion_finish    SDFAlgorithms::correctSDF(grid, correct_iterations) + clearInvalidVoxels (sdf/algorithms.cpp:260-366); count = saved voxels
 * i3d_fusion_get/save  the records in the order SparseVoxelGrid::save writes them (the reference's unordered_map iteration order) */
typedef struct i3d_fusion i3d_fusion;
int  i3d_fusion_create(int32_t device_ordinal, float voxel_size, float depth_min, float depth_max, const float* clip6, uint64_t initial_capacity, i3d_fusion** out);
void i3d_fusion_destroy(i3d_fusion* f);
const char* i3d_fusion_last_error(const i3d_fusion* f);
int  i3d_fusion_integrate(i3d_fusion* f, int32_t depth_w, int32_t depth_h, const float* depth_intr4, int32_t color_w, int32_t color_h, const float* color_intr4,
                          const float* depth, const uint8_t* bgr, const float* pose_cam_to_world16, int32_t erode_window);
int  i3d_fusion_finish(i3d_fusion* f, int32_t correct_iterations, uint64_t* count);
int  i3d_fusion_info(const i3d_fusion* f, uint64_t* frames, uint64_t* allocated, uint64_t* capacity, int32_t* correct_launches);
int  i3d_fusion_get(const i3d_fusion* f, int32_t* keys, float* sdf, float* weight, uint8_t* color);
int  i3d_fusion_save(const i3d_fusion* f, const char* path);

/* ---- resume a volume: records into an empty volume, a volume from a .tsdf, the records of an open volume.
 * i3d_fusion_insert_records  SparseVoxelGrid::load's loop data_[key] = voxel (sparse_voxel_grid.cpp:532-569) on an empty volume.
 *  1. The volume must be empty and untouched (frames == 0, no stored voxel): a second load, a load after any integrate or merge, and a load after
 *     i3d_fusion_finish are I3D_ERR_STATE.
 *  2. Record i is stored as given - sdf, weight and colour (R,G,B as i3d_fusion_get) bit for bit - records of weight 0 included (allocated, empty).  The clip box
 *     is not applied to loaded records (the reference's load ignores it); it goes on applying to later allocation.
 *  3. The rank of record i is (0 << 41) | i: the load consumes ordinal 0, which is never live (i3d_fusion_deintegrate(0, ..) is I3D_ERR_STATE), and `frames` becomes
 *     1 even for n == 0.  i3d_fusion_debug_voxels reports first_frame 0 for loaded voxels; the next integrate has ordinal 1 and sees them as earlier.  A loaded voxel
 *     has never been a block centre, so a later frame inserts what is missing around it.
 *  4. The record order of everything later (snapshot, finish, save) is the reference's after load then integrate: the iteration order of an unordered_map that
 *     received the records in file order, then the later insertions.  This is NOT the file's own order: the reference reorders on load, and so does this.
 *  5. I3D_ERR_INVALID_ARGUMENT, checked before anything is written: a null handle; null keys / sdf / weight / color with n > 0; n > 2^30; any |key| >= 2^20; a
 *     non-finite sdf; a non-finite or negative weight.  A key that appears twice is I3D_ERR_INVALID_ARGUMENT too (found on the device: fewer voxels stored than
 *     records); the volume is emptied again and a correct load succeeds afterwards.  I3D_ERR_CAPACITY as a growing i3d_fusion_integrate.  n == 0 is I3D_OK.
 *     The cached brick bitmap is dropped.
 * i3d_fusion_load      SparseVoxelGrid::create(filename, depth_min, depth_max) (sparse_voxel_grid.cpp:68-80): the header and records of the .tsdf, a handle with the
 *     file's voxel size, TRUNCATION and INTEGRATION WEIGHT SAMPLE (both feed integrate), then i3d_fusion_insert_records.  A file written with a weight sample of
 *     0 (i3d_tsdf_write's callers that have none) loads, and later frames integrate with unit weights: the reference's behaviour.  I3D_ERR_IO for a missing or
 *     truncated file and for a header with voxel size <= 1e-5, a non-finite or <= 0 truncation or a non-finite weight sample; I3D_ERR_NO_DEVICE as
 *     i3d_fusion_create; the record errors above.  On any error *out = NULL and nothing leaks.
 * i3d_fusion_snapshot  the records i3d_fusion_finish(f, 0, ..) would produce, WITHOUT closing the volume: the stored slots by rank, the replay, clearInvalidVoxels'
 *     selection (weight > 0), the export.  Nothing is written into the table and the brick bitmap is neither built nor dropped.  After a snapshot i3d_fusion_get /
 *     i3d_fusion_save return those records (I3D_ERR_STATE on a volume neither finished nor snapshotted); a later integrate does not invalidate them - they are
 *     replaced by the next snapshot or by finish.  On a finished volume: I3D_OK and the finished count.
 * Limits.  (1) A saved volume has lost its weight-0 voxels and its frame history: frames fused before the checkpoint cannot be deintegrated after a load.
 * (2) The record order after a load is the reference's after load, not that of an uninterrupted run, so correctSDF (a Gauss-Seidel sweep in that order) may give
 * other values than an uninterrupted run; equality with an uninterrupted run is promised for the live state and for finish(0) as a set of records.  (3) Records
 * enter an empty volume only; two populated volumes are combined by i3d_fusion_merge. */
int  i3d_fusion_insert_records(i3d_fusion* f, uint64_t n, const int32_t* keys /*[n][3]*/, const float* sdf, const float* weight, const uint8_t* color /*[n][3] R,G,B*/);
int  i3d_fusion_load(int32_t device_ordinal, const char* path, float depth_min, float depth_max, const float* clip6, i3d_fusion** out);
int  i3d_fusion_snapshot(i3d_fusion* f, uint64_t* count);

/* ---- a fused frame taken out again, or moved to a corrected pose.  Every successful i3d_fusion_integrate has an ordinal: the value of
 * i3d_fusion_info's `frames` before the call (frames counts integrate operations and is never decremented).
 * i3d_fusion_deintegrate  removes the contribution frame `ordinal` made: the same upload, erosion, normals and frustum bounds as integrate, no allocation, then one
 *                         pass over the table.  A voxel changes only if the frame's gates pass AND the voxel was first inserted by this frame or an earlier one; a
 *                         voxel whose weight falls below 0.5 is an empty Voxel() again (it stays allocated; i3d_fusion_finish drops it).  The record order of a
 *                         volume saved afterwards is that of the table's whole insertion history, not of a volume that never saw the frame.
 * i3d_fusion_reintegrate  the frame taken out at old_pose and put in at new_pose in ONE pass over the table; bit-identical to i3d_fusion_deintegrate followed by
 *                         i3d_fusion_integrate at new_pose.  The frame's new ordinal (= frames before the call) goes to *new_ordinal (may be NULL).
 * Errors through i3d_fusion_last_error, nothing written on error: I3D_ERR_INVALID_ARGUMENT as i3d_fusion_integrate; I3D_ERR_STATE for an ordinal that is not in the
 * volume (never integrated, or already taken out) and after i3d_fusion_finish.
 * The caller must pass the depth, colour, intrinsics, pose and erode_window the frame was fused with.  Other values are NOT detected: the result is a wrong but
 * finite volume (weights cannot go negative, nothing faults). */
int  i3d_fusion_deintegrate(i3d_fusion* f, uint64_t ordinal, int32_t depth_w, int32_t depth_h, const float* depth_intr4, int32_t color_w, int32_t color_h,
                            const float* color_intr4, const float* depth, const uint8_t* bgr, const float* pose_cam_to_world16, int32_t erode_window);
int  i3d_fusion_reintegrate(i3d_fusion* f, uint64_t ordinal, int32_t depth_w, int32_t depth_h, const float* depth_intr4, int32_t color_w, int32_t color_h,
                            const float* color_intr4, const float* depth, const uint8_t* bgr, const float* old_pose_cam_to_world16, int32_t erode_window,
                            const float* new_pose_cam_to_world16, uint64_t* new_ordinal);

/* ---- one volume fused into another under a rigid motion: f <- f (+) T(src), the running weighted mean with a whole volume as the sample.
 * pose6 = angle-axis | t maps src's world to f's world, x_f = R x_src + t: exactly the pose i3d_fusion_register_points(f, points in src's frame) returns; NULL =
 * identity.  i3d_fusion_register_volume(f, src) below finds that pose from the two volumes themselves.  Every lattice point k of f whose sample from src is defined receives it, stored before or not (a new voxel is inserted subject to f's clip box and
 * only if it receives a sample).
 *   general path  the sample at p = R^T (k voxel_size - t) is defined where the cell of i3d_fusion_query_points in src is valid (8 corners stored with weight != 0):
 *                 the trilinear sdf, the trilinear weight, the trilinear colour rounded to nearest, all in fp64
 *   aligned path  runs when pose6 is NULL, or its three rotation entries are 0 and every t[a] / voxel_size is an integer m[a] of magnitude < 2^20: the sample of k
 *                 is the src voxel k - m (stored with weight != 0) as it is, no neighbours required - exact, and it keeps src's outer layer
 * The sample enters a voxel exactly as a frame's sample does (integrate's update).  A successful merge consumes one ordinal (`frames` before the call), which is
 * never live: i3d_fusion_deintegrate of it is I3D_ERR_STATE.  Taking out an earlier frame skips the voxels the merge inserted; a later integrate feeds them.
 * src is read as it stands, before or after i3d_fusion_finish, and is left bit-identical (its cached brick bitmap may be built); f's cached bitmap is dropped.
 * Errors through i3d_fusion_last_error(f), nothing written: I3D_ERR_INVALID_ARGUMENT for a null handle, f == src, volumes on different devices, voxel_size or
 * truncation not bitwise equal, a non-finite pose; I3D_ERR_STATE after i3d_fusion_finish of f; I3D_ERR_CAPACITY as a growing i3d_fusion_integrate.  An empty src
 * is I3D_OK: zero counts, the ordinal consumed, the table untouched.
 * Limits: a src voxel that received depth but never colour counts as black (as section 22); merged-in content cannot be taken out again; both volumes must share
 * the voxel size. */
typedef struct {
    uint64_t ordinal;            /* the ordinal this merge consumed (= frames before the call) */
    int64_t  source_voxels;      /* slots of src stored with weight != 0 */
    int64_t  sampled;            /* voxels of f that received a sample */
    int64_t  allocated;          /* of those, newly inserted into f */
    int32_t  aligned;            /* 1: the aligned path ran */
    int32_t  pad;
    double   rotation[9], translation_voxels[3];   /* the motion exactly as the kernels used it: row-major R, t / voxel_size */
} i3d_merge_stats;
int  i3d_fusion_merge(i3d_fusion* f, i3d_fusion* src, const double* pose6 /* NULL = identity */, i3d_merge_stats* stats /* may be NULL */);

/* ---- stored voxels dropped by weight, distance or box (none in the reference, whose fusion grid only grows until clearInvalidVoxels).
 * A stored voxel with key (x, y, z), sdf s and weight w FAILS a criterion as follows, all in float exactly as written:
 *   W  enabled when min_weight >= 0:   !(w > min_weight)
 *   S  enabled when max_abs_sdf > 0:   fabsf(s) > max_abs_sdf
 *   B  enabled when box_mode != 0:     with wx = (float)x * voxel_size (wy, wz likewise) the voxel is outside iff wx < box6[0] || wx > box6[1] || .. - the clip
 *                                      test of the allocation, faces inclusive; box_mode 1 keeps the inside (fails when outside), 2 erases it (fails when inside)
 * and it is removed iff it fails at least one enabled criterion.  With min_weight = 0 and the rest off the call removes exactly the weightless voxels: what
 * allocation made and no frame fed, and what i3d_fusion_deintegrate emptied.
 * counts5 = {stored before, removed, failed W, failed S, failed B}; a voxel failing several criteria counts in each.  Written on success, also when nothing goes.
 * Nothing removed: the table is not touched at all, no cache is dropped, shrink is ignored.  Otherwise the survivors move into a fresh table (no tombstones) with
 * key, sdf, weight, colour and first-insertion rank bit for bit; the capacity is unchanged, or with shrink != 0 that of i3d_fusion_create for initial_capacity =
 * survivors (the smallest power of two >= 4096 with capacity >= 2 survivors), never above the current one.  A later frame whose ray enters a survivor expands its
 * 3x3x3 block again and inserts what is missing around it with that frame's ranks; where nothing is missing this inserts nothing.  The call consumes no ordinal:
 * `frames` and the live frames are as before; taking out a live frame later skips the voxels that are gone and treats survivors as before; a removed voxel that a
 * later frame inserts again carries that frame's ordinal.  The insertion sequence afterwards is the old one less the removed keys, and snapshot / finish replay
 * it: the ORDER of the records may differ from the unpruned volume's even when only weightless voxels went, their SET does not in that case.  The records of an
 * earlier snapshot are kept, as i3d_fusion_integrate keeps them.  The cached brick bitmap is dropped when anything was removed.
 * Errors through i3d_fusion_last_error, nothing written: I3D_ERR_INVALID_ARGUMENT for a null handle, a non-finite min_weight or max_abs_sdf, box_mode outside
 * 0..2, box_mode != 0 with a null or non-finite box or lo > hi on an axis; I3D_ERR_STATE after i3d_fusion_finish; I3D_ERR_HIP if the new table cannot be
 * allocated (the old one stays intact).
 * Limits: no criterion on age (only the first-insertion rank is stored) and none on connected components here (i3d_fusion_prune_components below);
 * what is removed comes back only by fusing again; a frame fused before a prune and taken out after it no longer touches the removed voxels. */
int  i3d_fusion_prune(i3d_fusion* f, float min_weight, float max_abs_sdf, int32_t box_mode, const float* box6 /* {x0,x1,y0,y1,z0,z1}, metres, as clip6 */,
                      int32_t shrink, int64_t* counts5 /* may be NULL */);

/* ---- connected components of the stored voxels: label and drop floaters (none in the reference, which cleans the downloaded mesh only).
 * NODE: a stored voxel that passes criteria W and S of i3d_fusion_prune above, compared in float exactly as written there: W enabled when min_weight >= 0, passed
 * iff w > min_weight; S enabled when max_abs_sdf > 0, passed iff !(fabsf(s) > max_abs_sdf); with both off every stored voxel is a node.  EDGE: two nodes whose
 * keys differ by exactly 1 on exactly one axis (6-connectivity).  Components are numbered by descending size (number of nodes), ties by ascending smallest packed
 * key (z, then y, then x) among their nodes.  Nodes are listed in ascending packed key; label[i] is the number of the component of node i, sizes[c] the size of
 * component c.  Nothing depends on capacity, growth history, slot layout or timing: two runs give the same bits.
 * i3d_fusion_components reads the table as it stands, before or after i3d_fusion_finish, and changes nothing another entry point reads (no ordinal, the brick
 * bitmap neither built nor dropped).  counts3 = {nodes, components, size of the largest}; no node is I3D_OK with {0, 0, 0}.  The labelling is kept in the handle
 * as host copies until the next i3d_fusion_components or the destroy, also across calls that change the volume; i3d_fusion_get_components copies it out (any
 * pointer may be NULL) and is I3D_ERR_STATE before any labelling.  More than 2^31 - 1 nodes: I3D_ERR_CAPACITY.
 * i3d_fusion_prune_components labels afresh with the same two criteria (the handle's stored labelling is left alone) and removes every node of a component c with
 *   (min_voxels > 0 && sizes[c] < min_voxels) || (keep_largest > 0 && c >= keep_largest)
 * Stored voxels that are not nodes are neither labelled nor removed (i3d_fusion_prune handles those; with S on, the far-band voxels of a removed floater stay).
 * counts5 = {stored before, voxels removed, nodes, components, components removed}, may be NULL.  Everything else is i3d_fusion_prune with this verdict: nothing
 * removed = table untouched; survivors keep key, sdf, weight, colour and rank bit for bit and move into a fresh table of the same or (shrink) the shrunk
 * capacity; later frames re-expand blocks around survivors; no ordinal is consumed; the insertion sequence is the old one less the removed keys; the brick bitmap
 * is dropped when something was removed; I3D_ERR_STATE after i3d_fusion_finish.
 * Errors through i3d_fusion_last_error, nothing written: I3D_ERR_INVALID_ARGUMENT for a null handle, a non-finite min_weight or max_abs_sdf, a negative
 * min_voxels or keep_largest, a null counts3; I3D_ERR_HIP also when a bounded loop of the union-find ran out (no labelling then).
 * Relation to i3d_fusion_extract_mesh (min_weight = 0 on both sides, weights >= 0): the owner voxels of a face's three vertices carry one label, so every
 * connected component of the mesh lies inside one voxel component.  Not the converse: two surfaces closer than twice the truncation share a band and are one
 * component unless max_abs_sdf parts them. */
int  i3d_fusion_components(i3d_fusion* f, float min_weight, float max_abs_sdf, int64_t* counts3 /* nodes, components, size of the largest */);
int  i3d_fusion_get_components(i3d_fusion* f, int32_t* keys /*[nodes][3]*/, int32_t* label /*[nodes]*/, int64_t* sizes /*[components]*/);   /* any may be NULL */
int  i3d_fusion_prune_components(i3d_fusion* f, float min_weight, float max_abs_sdf, int64_t min_voxels, int64_t keep_largest, int32_t shrink, int64_t* counts5);

/* ---- the fusion volume as a model while it is being fused.  Both read the table as it stands, before or after i3d_fusion_finish,
 * and change nothing in it: integrate / finish / get / save results are bit-identical with calls in between.  The brick bitmap of the empty-space skipping is
 * cached in the handle and dropped by i3d_fusion_integrate and i3d_fusion_finish.  Errors through i3d_fusion_last_error: I3D_ERR_INVALID_ARGUMENT for a null
 * handle / descriptor / pose / depth, frame != -1, use_context_camera != 0 and the range checks of i3d_render_view / i3d_track_frame; I3D_ERR_CAPACITY when the
 * bitmap of the volume's bounding box would exceed 2^31 bits.  An empty volume has no bricks: no hits, and tracking gives status 2. */
/* the ray cast of i3d_render_view (section 13.1) over the volume: cells whose 8 corners are stored with weight != 0, trilinear fused sdf.
 * desc->frame must be -1 (free camera); use_refined_sdf is ignored (the volume has one field).  depth / normal as i3d_render_view; either may be NULL. */
int i3d_fusion_render(i3d_fusion* f, const i3d_render_desc* desc, float* depth, float* normal, i3d_render_stats* stats);
/* i3d_track_frame (section 14.1) with the volume as the model; desc->use_context_camera must be 0 (the intrinsics are the depth camera's),
 * use_refined_sdf is ignored.  A volume with nothing to associate against (e.g. before the first integrate) gives status 2 and the pose unchanged. */
int i3d_fusion_track(i3d_fusion* f, const i3d_track_desc* desc, int32_t width, int32_t height, const float* depth, double* pose6_io, i3d_track_stats* stats);

/* ---- the model at arbitrary world points: value, unit gradient, albedo, and the foot of the gradient path on the zero level set (DESIGN.md section 17
 * defines every output).  A point p has q = p / voxel_size; its cell is the one of i3d_render_view (all 8 corners stored with weight != 0), the value the trilinear
 * interpolant there.  With project = 1 the point walks p <- p - clamp(f vs / |g|, -vs, vs) g / |g| until |f| <= tolerance_voxels * vs (tested before each
 * step), at most max_steps steps; it stops without a foot when an iterate's cell is not valid or |g| = 0.  This is the foot of the gradient path, not the exact
 * closest point.  status[i] bit 0: the cell at p is valid (sdf, normal, albedo meaningful); bit 1: foot and distance = sign(sdf) |foot - p| meaningful; every
 * output of an unset bit is 0.  A point with a non-finite coordinate or any |q| >= 2^20 is invalid.  Changes nothing any other entry point reads. */
typedef struct {
    int32_t use_refined_sdf;     /* 1: sdf_refined, 0: the fused sdf (as i3d_render_view); ignored by i3d_fusion_query_points */
    int32_t project;             /* 1: walk onto the zero level set (foot, distance) */
    int32_t max_steps;           /* 0..64 */
    double  tolerance_voxels;    /* > 0, finite */
} i3d_query_desc;

/* counts, and sums over the points with status bit 0 (sdf) / bit 1 (distance).  Summed on the device in a fixed order: the same input gives the same bits.
 * steps: Newton steps taken by all points together. */
typedef struct {
    int64_t valid, projected;
    double  sum_abs_sdf, sum_sq_sdf, max_abs_sdf;
    double  sum_abs_distance, sum_sq_distance, max_abs_distance;
    int64_t steps;
} i3d_query_stats;

void i3d_query_desc_default(i3d_query_desc* d);      /* refined, project = 1, max_steps = 16, tolerance_voxels = 1e-6 */
/* points: [n][3] world, n <= 2^27.  Every output may be NULL; foot / distance need project = 1.  n = 0 succeeds with zero stats. */
int  i3d_query_points(i3d_context* ctx, const i3d_query_desc* desc, int64_t n, const double* points,
                      double* sdf, float* normal /*[n][3]*/, float* albedo, double* foot /*[n][3]*/, double* distance, uint8_t* status, i3d_query_stats* stats);
/* the same over the fusion volume as it stands, before or after i3d_fusion_finish (the cell of i3d_fusion_render: float sdf widened to fp64; no albedo);
 * errors through i3d_fusion_last_error */
int  i3d_fusion_query_points(i3d_fusion* f, const i3d_query_desc* desc, int64_t n, const double* points,
                             double* sdf, float* normal /*[n][3]*/, double* foot /*[n][3]*/, double* distance, uint8_t* status, i3d_query_stats* stats);

/* ---- the caller's own rays on the model (DESIGN.md section 34 defines every output).  Ray i has the origin o = origins[i] and the direction d = directions[i],
 * both world, metres; d need not be unit.  Its parameter t is in units of d: the point at t is o + t d, and the ray is marched over [a, b) with a = t_min[i]
 * (t_min NULL or t_min[i] <= 0: 0) and b = t_max[i] (t_max NULL or t_max[i] <= 0: +inf), the renderer's "<= 0: open" rule per ray.  Everything else is the march
 * of i3d_render_view (section 13.1 items 2-5: cells, brick bitmap, steps, the budget of 2^14 samples, the two secant steps at the first zero crossing from
 * outside) with eye = o and dir = d: the rays d = R^T (x, y, 1) of a pinhole camera give that view's depth as t, bit for bit.
 * VISIBILITY: the segment A -> B is occluded iff the ray o = A, d = B - A, t_max = 1 hits.
 * A ray is invalid, and never marched, when a component of o or d is not finite, t_min[i] or t_max[i] is NaN, t_min[i] = +inf, the squared length
 * (dx^2 + dy^2) + dz^2 is 0 or not finite, or any |o[a] / voxel_size| >= 2^20 (the bound of i3d_query_points).
 * Outputs, [n] or [n][3], any may be NULL: t = the hit's parameter; position = o + t d; normal, albedo, shading, intensity as i3d_render_view at the hit;
 * status bit 0: the ray was valid and marched, bit 1: hit, bit 2: the march used its 2^14 samples without a hit.  Every output of a ray without a hit is 0, every
 * output of an invalid ray is 0.  stats (may be NULL): hits and samples as i3d_render_view, residual_sq_sum = 0.
 * order: 0 marches the rays in the order given; 1 sorts them on the device by direction octant and entry brick first, so that the rays of a wave walk the same
 * bricks.  The order changes which lane marches a ray and nothing else: every output and both stats are bit-identical.  Measured (DESIGN.md
 * 34.3): it pays from about 10^6 rays, the more the less coherent they come; at 3 10^5 rays and below the sort costs more than it saves.
 * THE LIMIT: a ray that starts inside the surface has no hit until it has left it and meets a zero crossing from outside (13.1 item 4); a ray that starts in
 * cells that are not stored sees nothing there.
 * Reads and writes as i3d_render_view: the grid and the per-voxel SH are read, the cached brick bitmap is built or reused, nothing any other entry point reads
 * is changed.  Errors, with nothing written: I3D_ERR_INVALID_ARGUMENT for a null handle, n < 0 or n > 2^27, NULL origins / directions with n > 0, order outside
 * 0 / 1; I3D_ERR_STATE without a grid, or when shading / intensity are requested without the per-voxel SH; I3D_ERR_CAPACITY from the bitmap, as
 * i3d_render_view.  n = 0 succeeds with zero stats. */
int i3d_cast_rays(i3d_context* ctx, int32_t use_refined_sdf, int32_t order, int64_t n,
                  const double* origins, const double* directions, const double* t_min, const double* t_max,
                  double* t, double* position, float* normal, float* albedo, float* shading, float* intensity,
                  uint8_t* status, i3d_render_stats* stats);
/* the same over the fusion volume as it stands, before or after i3d_fusion_finish (the cells of i3d_fusion_render; no albedo or SH); errors through
 * i3d_fusion_last_error */
int i3d_fusion_cast_rays(i3d_fusion* f, int32_t order, int64_t n,
                         const double* origins, const double* directions, const double* t_min, const double* t_max,
                         double* t, double* position, float* normal, uint8_t* status, i3d_render_stats* stats);

/* ---- the stored colour at the hit: colour planes for views and for the caller's rays (DESIGN.md section 35 defines it).  The context holds one colour per voxel
 * (i3d_grid_view::color, i3d_update_grid, i3d_recompute_colors), the fusion volume one per table slot.  The colour at a hit is taken in the cell the siblings'
 * normal and albedo are taken in (the cell of the hit, or of the hit sample when the hit's is not valid): per channel the eight corners' stored bytes, widened to
 * fp64, under the trilinear weights of the hit - albedo's expression in albedo's order.  The unit is the stored byte, 0..255, unrounded float; the channels are
 * R, G, B in every output.  A pixel or ray without a hit gets 0, 0, 0.  A fusion voxel that received depth but never colour counts as black.
 * use_refined_sdf chooses the field that is marched; the colour is the one stored colour either way.  No per-voxel SH is read.
 * color: [h][w][3] or [n][3]; depth, t, status and the stats are those of i3d_render_view / i3d_fusion_render / i3d_cast_rays / i3d_fusion_cast_rays on the
 * same input, bit for bit; residual_sq_sum = 0.  Any output may be NULL.  i3d_render_view_color takes frame >= 0 (the keyframe's pose, the level's
 * intrinsics) as i3d_render_view does; the volume needs frame == -1.
 * Reads and writes as the siblings: the cached brick bitmap is built or reused, nothing any other entry point reads is changed.  Errors, with nothing written,
 * are the siblings' without those about the SH: I3D_ERR_INVALID_ARGUMENT for a null handle or descriptor, a frame / level / image size out of range, frame != -1
 * on the volume, n < 0 or n > 2^27, NULL origins / directions with n > 0, order outside 0 / 1; I3D_ERR_STATE without a grid (and, for a view with frame >= 0,
 * without keyframes or a camera); I3D_ERR_CAPACITY from the bitmap.  n = 0 succeeds with zero stats. */
int i3d_render_view_color(i3d_context* ctx, const i3d_render_desc* desc, float* color, float* depth, i3d_render_stats* stats);
int i3d_fusion_render_color(i3d_fusion* f, const i3d_render_desc* desc, float* color, float* depth, i3d_render_stats* stats);
int i3d_cast_rays_color(i3d_context* ctx, int32_t use_refined_sdf, int32_t order, int64_t n,
                        const double* origins, const double* directions, const double* t_min, const double* t_max,
                        double* t, float* color, uint8_t* status, i3d_render_stats* stats);
int i3d_fusion_cast_rays_color(i3d_fusion* f, int32_t order, int64_t n,
                               const double* origins, const double* directions, const double* t_min, const double* t_max,
                               double* t, float* color, uint8_t* status, i3d_render_stats* stats);

/* ---- rigid alignment of a point set to the model: Gauss-Newton on the stored field at the placed points, r_i = f(R p_i + t) (DESIGN.md section 18 defines
 * every figure).  pose6_io is angle-axis | t and maps the points' frame to the world, x = R p + t.  For the camera-frame points of a depth frame this is
 * camera -> world: the INVERSE of the world -> camera pose that i3d_track_frame takes.  A point counts (is valid) when its cell, the one of i3d_query_points, is
 * valid at the placed position; a valid point is an inlier when |f| <= max_distance.  The step solves the 6x6 system of J = [(x' x grad f)^T, grad f^T] about a
 * pivot fixed for the call (the placed mean of the points), T <- exp(delta) T; the loop stops after a step with |omega| < stop_rotation and |upsilon| <
 * stop_translation (status 0) or when the budget is used (status 1).  Every sum is formed on the device in a fixed order: the same input gives the same bits.
 * THE LIMIT: only points that land in a stored, valid cell contribute, so the basin is the stored band (the truncation of 5 voxels, less after
 * i3d_clear_outside_thin_shell).  This is fine registration: no global alignment, no scale estimation, no robust loss.
 * Errors: I3D_ERR_STATE without a grid; I3D_ERR_INVALID_ARGUMENT for a null pointer, n < 0 or n > 2^27, iterations outside 0..200, max_distance not finite or
 * <= 0, a non-finite pose.  n = 0 gives status 2.  Whenever no step was applied (status 2, iterations = 0, status 3 at the first step) pose6_io is left
 * unchanged bit for bit.  Changes nothing any other entry point reads. */
typedef struct {
    int32_t use_refined_sdf;     /* as i3d_query_desc; ignored by the fusion variant */
    int32_t iterations;          /* Gauss-Newton budget, 0..200 (0: only the figures at the given pose; status 1, or 2 below 64 inliers) */
    double  max_distance;        /* gate on |f| at the placed point, metres, > 0 */
    double  stop_rotation, stop_translation;   /* as i3d_track_desc */
} i3d_register_desc;

typedef struct {
    int32_t iterations;          /* steps applied */
    int32_t status;              /* 0 converged, 1 budget used, 2 fewer than 64 inliers (pose unchanged), 3 degenerate system (last good pose) */
    int64_t valid, inliers;      /* at the returned pose: points in a valid cell / of those with |f| <= max_distance */
    double  rms_initial, rms_final;            /* RMS of f over the inliers: at the given pose / at the returned pose */
    double  min_pivot_ratio;     /* as i3d_track_stats */
} i3d_register_stats;

void i3d_register_desc_default(i3d_register_desc* d);      /* refined, 30 iterations, max_distance 0.05 m, stop 1e-6 / 1e-6 */
/* points: [n][3] in their own frame, n <= 2^27; points with a non-finite coordinate, or placed at |x / voxel_size| >= 2^20, are ignored.  stats may be NULL. */
int  i3d_register_points(i3d_context* ctx, const i3d_register_desc* desc, int64_t n, const double* points /*[n][3]*/, double* pose6_io, i3d_register_stats* stats);
/* the same against the fusion volume as it stands, before or after i3d_fusion_finish (the cell of i3d_fusion_query_points); errors through i3d_fusion_last_error */
int  i3d_fusion_register_points(i3d_fusion* f, const i3d_register_desc* desc, int64_t n, const double* points, double* pose6_io, i3d_register_stats* stats);

/* ---- one fusion volume aligned to another on the two stored fields (DESIGN.md section 28 defines every figure): i3d_register_points with src's own voxels as the
 * points and the values src stores there as the targets, all on the device - nothing is extracted on the host and no point array is uploaded.
 *  1. pose6_io = angle-axis | t maps src's world to f's world, x_f = R x_src + t: exactly the pose i3d_fusion_merge takes.
 *  2. A slot of src is a sample when it is stored with weight != 0, fabs(sdf) <= source_band_voxels * src's voxel size, and every coordinate is a multiple of
 *     stride (negative coordinates included).  Its point is p = k * src's voxel size, its target the stored sdf s.
 *  3. The samples form one list in ascending packed key: the order of every sum depends on src's content alone, not on its table's capacity or slot layout.  More
 *     than 2^27 samples is I3D_ERR_CAPACITY (raise stride).
 *  4. The pivot is the placed mean of the samples, fixed for the call, as i3d_register_points.
 *  5. A sample is valid when the cell of i3d_fusion_query_points in f at x = R p + t is valid, an inlier when also |r| <= max_distance, r = f(x) - s in fp64.
 *  6. Step, loop, statuses (0 / 1 / 2 / 3, the 64-inlier floor) and "pose unchanged bit for bit when no step was applied" are those of i3d_register_points.  No
 *     sample at all (an empty src, a band that selects nothing) and an empty f give status 2.
 *  7. Every sum is formed on the device in a fixed order: the same two volumes give the same bits.
 *  8. Defaults: 30 iterations, stride 1, source_band_voxels 2.0, max_distance 0.05 m, stop 1e-6 / 1e-6.
 *  9. Both volumes are read as they stand, before or after i3d_fusion_finish, and left bit-identical; no ordinal is consumed, no cached brick bitmap is built or
 *     dropped.  Their voxel sizes and truncations may differ (points are metric, the band is in src's voxels).  Errors through i3d_fusion_last_error(f), nothing
 *     written: I3D_ERR_INVALID_ARGUMENT for a null handle / descriptor / pose, f == src, volumes on different devices, iterations outside 0..200, stride outside
 *     1..64, source_band_voxels or max_distance not finite or <= 0, a non-finite pose.
 * 10. LIMITS: this is fine registration.  The basin is the overlap of the two stored bands; there is no global alignment and no robust loss; the samples are
 *     unweighted (src's fusion weight selects, it does not weigh). */
typedef struct {
    int32_t iterations;          /* Gauss-Newton budget, 0..200 (0: only the figures at the given pose; status 1, or 2 below 64 inliers) */
    int32_t stride;              /* 1..64: the samples are the voxels whose three coordinates are multiples of it */
    double  source_band_voxels;  /* > 0, finite: |stored sdf| of a sample at most this many of src's voxels */
    double  max_distance;        /* gate on |r| = |f(x) - s|, metres, > 0 */
    double  stop_rotation, stop_translation;   /* as i3d_track_desc */
} i3d_register_volume_desc;

typedef struct {
    int32_t iterations, status;  /* as i3d_register_stats */
    int64_t valid, inliers;
    double  rms_initial, rms_final;            /* RMS of r over the inliers */
    double  min_pivot_ratio;
    int64_t selected;            /* samples: the length of the list */
} i3d_register_volume_stats;

void i3d_register_volume_desc_default(i3d_register_volume_desc* d);
int  i3d_fusion_register_volume(i3d_fusion* f, i3d_fusion* src, const i3d_register_volume_desc* desc, double* pose6_io, i3d_register_volume_stats* stats /* may be NULL */);

/* ---- an indexed, welded mesh of the volume as it stands, before or after i3d_fusion_finish (DESIGN.md section 29 defines every figure; tests/fusion_mesh_twin.py
 * states it in numpy).  Marching cubes over the fusion table; welding and degenerate-face removal run on the device, only the finished arrays are downloaded.
 *  1. The cell of lattice point k has the corners k + {0,1}^3 (the cell of i3d_fusion_query_points).  It is valid iff all 8 corners are stored with weight != 0 and
 *     weight >= min_weight and all 8 stored sdf values are finite (i3d_extract_mesh would emit NaN positions there).
 *  2. Configuration (sdf < 0), triangle table and triangle sequence of a cell are those of i3d_extract_mesh; the three corners of every triangle are the positions and
 *     colours i3d_extract_mesh(use_refined_sdf = 0, color_mode = 0) emits for that cell on a context that holds the same voxels, bit for bit.
 *  3. Weld = the reference's weld by position (+0 == -0), decided by naming instead of hashing: a triangle corner that lies on a lattice point is that voxel's corner
 *     vertex; any other is a vertex of its cell edge, and the two directions in which neighbouring cells walk an x or y edge are one vertex exactly where they give
 *     the same coordinate (the interpolation is not symmetric in the last bit; the reference leaves two vertices there, and so does this).  A corner vertex's colour
 *     is its voxel's stored colour, an edge vertex's the interpolated one of its direction.
 *  4. Order: vertices in ascending (packed key of the owner voxel - z, then y, then x -, code: corner, +x, +y, +z edge, descending twin of +x, of +y); faces by
 *     cell in ascending packed key, a cell's triangles in table order.  Nothing depends on the table's capacity, growth history or slot layout.
 *  5. A triangle with two equal indices or an area of 0 / NaN / inf (the fp32 expression of MeshUtil::removeDegenerateFaces) is dropped; its vertices stay.
 *  6. largest_component_only = 1 applies i3d_mesh_remove_loose_components to the downloaded mesh (host work).
 *  7. More than 2^31 - 1 vertices or face indices is I3D_ERR_CAPACITY; a volume with no valid cell or no surface cell is I3D_OK with zero counts.
 *  8. The table is read as it stands and left bit-identical; no ordinal is consumed and no cached brick bitmap is built or dropped.  The mesh lives in the handle:
 *     the next extract replaces it, i3d_fusion_destroy frees it; i3d_fusion_get_mesh before any extract is I3D_ERR_STATE.  Errors through i3d_fusion_last_error,
 *     nothing written: I3D_ERR_INVALID_ARGUMENT for a null handle or descriptor, a negative or non-finite min_weight, largest_component_only outside 0 / 1. */
typedef struct {
    float   min_weight;              /* >= 0, finite: a cell needs this fusion weight at all 8 corners (default 0: weight != 0 alone) */
    int32_t largest_component_only;  /* 0 / 1 (default 0) */
} i3d_fusion_mesh_desc;
typedef struct {                     /* filled before the largest-component step, except vertices and faces, which describe the returned mesh */
    int64_t stored;                  /* slots with weight != 0 */
    int64_t valid_cells, surface_cells, raw_triangles;
    int64_t vertices, corner_vertices, faces, degenerate_removed;
    int64_t rounded_corner_occurrences;   /* triangle corners that reach a lattice point by rounding, not through one of the interpolation's early returns */
} i3d_fusion_mesh_stats;
void i3d_fusion_mesh_desc_default(i3d_fusion_mesh_desc* d);          /* 0, 0 */
int  i3d_fusion_extract_mesh(i3d_fusion* f, const i3d_fusion_mesh_desc* desc, int64_t* num_vertices, int64_t* num_faces, i3d_fusion_mesh_stats* stats /* may be NULL */);
int  i3d_fusion_get_mesh(i3d_fusion* f, float* vertices /*[nv][3]*/, uint8_t* colors /*[nv][3] R,G,B*/, int32_t* faces /*[nf][3]*/);   /* any may be NULL */
/* extract + i3d_write_ply; I3D_ERR_STATE for an empty mesh.  Leaves the mesh i3d_fusion_get_mesh returns as it was. */
int  i3d_fusion_export_mesh_ply(i3d_fusion* f, const i3d_fusion_mesh_desc* desc, const char* path);

/* ---- registration of a depth frame on the stored field, no ray cast (DESIGN.md section 19 defines every figure): i3d_register_points on the back-projected
 * samples of the depth image, with the image in and the world -> camera pose of i3d_track_frame in and out (the driver inverts it on the host in both
 * directions).  The samples are the pixels (u, v) with u % stride == 0 and v % stride == 0; a sample is usable when its depth is finite, > 0 and inside
 * [min_depth, max_depth] where those are > 0; its point is depth * (x, y, 1) in fp64 with (x, y) the renderer's undistorted ray of the pixel.  The points are
 * formed inside the sums kernel and never stored.  With huber_delta = k > 0 an inlier's entries of J^T J and J^T r carry the weight 1 for |r| <= k, else
 * k / |r|; r^2 and the counts stay unweighted.  Pivot, residual, step, loop and statuses are those of i3d_register_points, and so is THE LIMIT: the basin is the
 * stored band.  Errors: I3D_ERR_STATE without a grid, or without a camera when use_context_camera = 1; I3D_ERR_INVALID_ARGUMENT for a null pointer, an image
 * edge <= 0 or > 32768, stride outside 1..16, iterations outside 0..200, max_distance not finite or <= 0, a non-finite huber_delta, a non-finite pose, a focal
 * length <= 0, use_context_camera != 0 on the fusion variant.  Whenever no step was applied pose6_io is left unchanged bit for bit.  Changes nothing any other
 * entry point reads. */
typedef struct {
    int32_t use_refined_sdf;     /* as i3d_register_desc; ignored by the fusion variant */
    int32_t use_context_camera;  /* as i3d_track_desc; must be 0 for the fusion variant */
    double  intrinsics4[4], distortion5[5];   /* level 0, colour geometry, when use_context_camera = 0 */
    int32_t iterations;          /* Gauss-Newton budget, 0..200 */
    int32_t stride;              /* 1..16: pixels (u, v) with u % stride == 0 and v % stride == 0 are used */
    double  max_distance;        /* gate on |f| at the placed point, metres, > 0 */
    double  huber_delta;         /* metres; <= 0: off (every inlier has weight 1) */
    float   min_depth, max_depth;/* as i3d_track_desc */
    double  stop_rotation, stop_translation;
} i3d_track_sdf_desc;

typedef struct {
    int32_t iterations, status;          /* as i3d_register_stats */
    int64_t valid_pixels, valid, inliers;/* sampled pixels with a usable depth / of those in a valid cell / of those inside the gate, at the returned pose */
    double  rms_initial, rms_final;      /* unweighted RMS of f over the inliers */
    double  min_pivot_ratio;
} i3d_track_sdf_stats;

void i3d_track_sdf_desc_default(i3d_track_sdf_desc* d);   /* refined, own camera, 30 iterations, stride 1, 0.05 m, huber off, depth range open, stop 1e-6 / 1e-6 */
/* depth: [height][width] metres, 0 = invalid.  pose6_io: world->camera, angle-axis | t, exactly as i3d_track_frame.  stats may be NULL. */
int  i3d_track_frame_sdf(i3d_context* ctx, const i3d_track_sdf_desc* desc, int32_t width, int32_t height, const float* depth, double* pose6_io,
                         i3d_track_sdf_stats* stats);
/* the same against the fusion volume as it stands, before or after i3d_fusion_finish; errors through i3d_fusion_last_error */
int  i3d_fusion_track_sdf(i3d_fusion* f, const i3d_track_sdf_desc* desc, int32_t width, int32_t height, const float* depth, double* pose6_io,
                          i3d_track_sdf_stats* stats);

/* ---- a batch of depth frames registered on the stored field in one loop.  Result b is what i3d_track_frame_sdf returns for frame b with
 * the same descriptor, bit for bit: the pose and every field of the stats, whatever the other frames of the batch are.  The return code is I3D_OK whatever the
 * frames' statuses are.  Errors as i3d_track_frame_sdf, with nothing written to the outputs; in addition I3D_ERR_INVALID_ARGUMENT for num_frames < 0 and for a
 * non-finite start pose in any frame.  num_frames == 0 is I3D_OK and touches nothing.  Changes nothing any other entry point reads. */
/* B frames of one size and one camera, depth[B][h][w] contiguous; poses6_io[B][6] world->camera in and out; stats[B] (may be NULL) */
int  i3d_track_frames_sdf(i3d_context* ctx, const i3d_track_sdf_desc* desc, int32_t num_frames, int32_t width, int32_t height,
                          const float* depth, double* poses6_io, i3d_track_sdf_stats* stats);
/* the context's resident keyframe depth of pyramid level `level`, no upload; frames[num] keyframe indices (NULL: 0..num-1, num must be K; indices may repeat).
 * The camera is the context's: its intrinsics x 2^-level, its distortion, the level's image size; desc->use_context_camera must be 1.  The start poses are the
 * caller's: the context's own poses are neither read nor written.  I3D_ERR_STATE without keyframes or without a camera; I3D_ERR_INVALID_ARGUMENT for a level or
 * a keyframe index out of range. */
int  i3d_track_keyframes_sdf(i3d_context* ctx, const i3d_track_sdf_desc* desc, int32_t level, int32_t num, const int32_t* frames,
                             double* poses6_io, i3d_track_sdf_stats* stats);

/* ---- the photometric term on the stored field (DESIGN.md section 21 defines every figure): i3d_track_frame_sdf with the model's appearance, still without a ray
 * cast and without an image gradient.  Per call one kernel turns the model into a per-voxel intensity c = albedo x SH shading at the voxel's normal (central
 * differences of the chosen field over the six axis neighbours; undefined where the voxel or one of the six has weight 0 or is not stored).  A geometric inlier
 * has a photometric sample when the eight c values of its cell are defined, its luminance is finite and |r_p| <= max_photo_residual where that is > 0; then
 * r_p = c(R p + t) - luminance(pixel), sampled with the trilinear weights of the geometric evaluation, and its Jacobian row is the geometric one with grad c in
 * place of grad f.  The system is geometric_weight^2 x the geometric one (Huber weight included) + photo_weight^2 x the photometric one; rms figures and counts
 * are unweighted.  Status 2: fewer than 64 geometric inliers when geometric_weight > 0, else fewer than 64 photometric samples.  With photo_weight = 0 no SH is
 * needed and no volume is built; with geometric_weight = 1 on top of that the pose and every base figure are i3d_track_frame_sdf's bit for bit.  luminance:
 * [height][width], the keyframes' convention, as i3d_track_frame_rgbd.  Errors: those of i3d_track_frame_sdf; I3D_ERR_INVALID_ARGUMENT for a null luminance, a
 * negative or non-finite weight, both weights 0, a non-finite max_photo_residual; I3D_ERR_STATE when photo_weight > 0 and the context has no per-voxel SH.  The
 * volume is built anew by every call: a call sees the fields as they stand.  Changes nothing any other entry point reads.
 * The fusion variant, i3d_fusion_track_sdf_rgbd, takes the volume's fused colour for the appearance: per call one kernel turns the table
 * into one value per slot, c = 0.114 b + 0.587 g + 0.299 r of the stored colour / 255 in fp32 (the keyframes' luminance), undefined where the slot is empty or has
 * weight 0; everything else is as above over the cell of i3d_fusion_track_sdf.  No SH is involved, so there is no I3D_ERR_STATE for it; use_context_camera must
 * be 0 and use_refined_sdf is ignored.  ITS LIMITS: a voxel that received depth but never colour (its projection missed the colour image) counts as black -
 * max_photo_residual is the caller's gate for it; no gain or bias between camera and volume; no coarse-to-fine schedule; no batch form. */
typedef struct {
    i3d_track_sdf_desc base;
    double  geometric_weight;    /* >= 0; default 1 */
    double  photo_weight;        /* >= 0, metres per unit luminance; default 0.1 */
    float   max_photo_residual;  /* gate on |r_p|; <= 0: open (default) */
    int32_t pad;
} i3d_track_sdf_rgbd_desc;

typedef struct {
    i3d_track_sdf_stats base;
    int64_t photo_samples;                       /* at the returned pose */
    double  photo_rms_initial, photo_rms_final;  /* unweighted RMS of r_p over the photometric samples */
} i3d_track_sdf_rgbd_stats;

void i3d_track_sdf_rgbd_desc_default(i3d_track_sdf_rgbd_desc* d);   /* i3d_track_sdf_desc_default, weights 1 and 0.1, gate open */
int  i3d_track_frame_sdf_rgbd(i3d_context* ctx, const i3d_track_sdf_rgbd_desc* desc, int32_t width, int32_t height, const float* depth, const float* luminance,
                              double* pose6_io, i3d_track_sdf_rgbd_stats* stats);
/* the same against the fusion volume as it stands, before or after i3d_fusion_finish, with the luminance of its fused colour; errors through
 * i3d_fusion_last_error: those of i3d_fusion_track_sdf and the argument errors above, nothing written to the outputs on error */
int  i3d_fusion_track_sdf_rgbd(i3d_fusion* f, const i3d_track_sdf_rgbd_desc* desc, int32_t width, int32_t height, const float* depth, const float* luminance,
                               double* pose6_io, i3d_track_sdf_rgbd_stats* stats);
/* the batch forms, with the contract of i3d_track_frames_sdf / i3d_track_keyframes_sdf: result b is the single call's on frame b bit for bit, the three
 * photometric figures included, whatever the chunking.  luminance[B][h][w] beside depth[B][h][w]; the keyframe form reads the resident depth AND luminance of
 * the level, no upload. */
int  i3d_track_frames_sdf_rgbd(i3d_context* ctx, const i3d_track_sdf_rgbd_desc* desc, int32_t num_frames, int32_t width, int32_t height,
                               const float* depth, const float* luminance, double* poses6_io, i3d_track_sdf_rgbd_stats* stats);
int  i3d_track_keyframes_sdf_rgbd(i3d_context* ctx, const i3d_track_sdf_rgbd_desc* desc, int32_t level, int32_t num, const int32_t* frames,
                                  double* poses6_io, i3d_track_sdf_rgbd_stats* stats);

/* ---- one process per GPU: the voxel state is replicated; row work / row storage / solver vectors are sharded by contiguous, tile-aligned
 * ranges of the brick-ordered work list (compact regions of the surface).  A rank builds rows for its range + a thin rim of ghost entries;
 * per PCG pass it pushes the operator input of the rim to its neighbours and joins ONE small all-reduce [camera block | p.q] plus the 4 iteration
 * scalars — over peer-to-peer xGMI mailboxes (self-tested at start-up), RCCL as the fallback and for the rare large collectives.  Call after i3d_create on every rank with the same unique id (i3d_comm_unique_id on rank 0,
 * broadcast by the launcher, e.g. torch.distributed). */
int i3d_comm_unique_id(void* out128, int32_t* bytes);
int i3d_comm_init(i3d_context* ctx, int32_t rank, int32_t world, const void* unique_id, int32_t id_bytes);
/* single-GPU simulation of W ranks (W host threads, one context each, same device) — test vehicle for the SPMD control flow */
void* i3d_comm_sim_create(int32_t world);
void  i3d_comm_sim_destroy(void* shared);
int   i3d_comm_init_sim(i3d_context* ctx, void* shared, int32_t rank);
/* host-side view of the sharding plan (no device needed): owned range and vector layout of `rank`, and which work-list entries
 * it must compute rows for.  anbr: [18][A] neighbour table in work-list space (-1 = none), active: [A]. */
int   i3d_shard_plan(int32_t A, int32_t world, int32_t rank, const int32_t* anbr, const uint8_t* active,
                     int32_t* chunk, int32_t* own0, int32_t* own1, uint8_t* in_compute_list /*[A]*/);
int32_t i3d_shard_vec_index(int32_t a, int32_t chunk, int32_t albedo);
/* need[e] bit k: rank k's rows read the unknowns of work-list entry e, which it does not own (what Comm::push_halo moves once per PCG pass) */
int   i3d_shard_need(int32_t A, int32_t world, const int32_t* anbr /*[18][A]*/, const uint8_t* active /*[A]*/, uint64_t* need /*[A]*/);
/* traffic log of the sharded path since i3d_comm_init: halo exchanges (calls, bytes this rank sent), all-reduces (calls, bytes), and the
 * plan of the last outer iteration (rim entries sent / received per pass, foreign tiles with ghost entries, compute-list length) */
int   i3d_comm_stats(i3d_context* ctx, int64_t* halo_calls, int64_t* halo_bytes_sent, int64_t* reduce_calls, int64_t* reduce_bytes,
                     int32_t* halo_entries_send, int32_t* halo_entries_recv, int32_t* ghost_tiles, int32_t* compute_list);
/* what carries the per-pass exchanges: "p2p-mailbox" (peer-to-peer stores over xGMI), "rccl" (fallback), "sim-*" (1-GPU rank simulation), "" without a communicator */
const char* i3d_comm_transport(i3d_context* ctx);

/* ---- measurement: HIP-event time (ms) and launch count accumulated per kernel family on the context's stream
 * since the last reset.  names: see i3d_kernel_name(). */
enum { I3D_K_CLASSIFY = 0, I3D_K_OBSERVE, I3D_K_BUILD, I3D_K_EG_PASS /* J^T W J p passes of the PCG */, I3D_K_GATHER, I3D_K_COST, I3D_K_VECTOR, I3D_K_SH,
       I3D_K_EG_AUX /* gradient and column-norm passes over the rows */,
       I3D_K_COMM /* sharded runs: halo push, all-reduce, all-gather launches (GPU time incl. waiting for the peers) */,
       I3D_K_EG_MR2, I3D_K_EG_MR3 /* operator passes of a ladder batch that serve 2 / 3 systems with one stream of the rows (I3D_K_EG_PASS: one system) */, I3D_K_COUNT };
int i3d_timing_enable(i3d_context* ctx, int32_t on);
/* restrict the per-launch HIP events to the categories of the mask (bit = 1 << I3D_K_*; default: all).  An event pair around EVERY launch of a
 * Gauss-Newton iteration (~900 launches) costs ~8 % of its wall clock; bench.py times only what its roofline needs. */
int i3d_timing_select(i3d_context* ctx, uint32_t category_mask);
int i3d_timing_get(i3d_context* ctx, double* ms /*[I3D_K_COUNT]*/, int64_t* launches /*[I3D_K_COUNT]*/, int32_t reset);
/* the same restricted to launches that did work: PCG launches queued behind the device-side convergence flag return at once (~4 us) and
 * would flatter an average; a launch counts when it lasted >= 25 % of the longest launch of its category */
int i3d_timing_get_work(i3d_context* ctx, double* ms /*[I3D_K_COUNT]*/, int64_t* launches /*[I3D_K_COUNT]*/);
/* the same, plus what the upper cut-off removed: launches that lasted more than 4x the 90th percentile of their category (a launch that straddles a
 * hiccup of the device) — their number and total time, so that a caller can quote them beside the average.  The exchange category is never cut. */
int i3d_timing_get_work_ex(i3d_context* ctx, double* ms, int64_t* launches, double* slow_ms /*[I3D_K_COUNT]*/, int64_t* slow_launches /*[I3D_K_COUNT]*/);
const char* i3d_kernel_name(int32_t k);
/* sizes of the last assembled problem: active voxels, Eg/Er/Es/Ea rows, free parameters */
int i3d_problem_sizes(i3d_context* ctx, int64_t out[6]);

/* ---- parity probes (tests only): assemble the rows of outer iteration `iteration` without solving and export them.
 * Arrays are indexed by visit order; slot k in [0, slots).  Any pointer may be NULL. */
int i3d_debug_assemble(i3d_context* ctx, const i3d_optimizer_config* cfg, int32_t iteration, int32_t* slots_out);
/* iteration order of the reference's unordered_map<Vec3i,...> after `map[key_i] = i`, i = 0..n-1: mode 0 = the host replay (repeated keys
 * allowed), 1 = the replay for distinct keys, 2 = a real std::unordered_map, 3 = the per-rehash-epoch closed form on the host, 4 = the same on
 * the current device (what the level transitions and the fusion volume use; distinct keys); returns the number of elements, -1 on error */
int64_t i3d_debug_map_order(const int32_t* keys, int64_t n, int32_t mode, int32_t* order);
int i3d_debug_flags(i3d_context* ctx, uint8_t* flags /*[N]: bit0 valid,1 active,2 ring_ok,3 free_sdf,4 free_albedo*/);
int i3d_debug_eg_rows(i3d_context* ctx, int32_t* frame /*[N][slots], -1 = none*/, float* weight /*[N][slots] normalised*/,
                      float* residual /*[N][slots]*/, float* jac /*[N][slots][29]*/);
int i3d_debug_reg_rows(i3d_context* ctx, uint8_t* has_er /*[N]*/, uint8_t* has_es /*[N]*/, float* ea_weight /*[N][6] normalised, 0 = none*/);
int i3d_debug_neighbors(i3d_context* ctx, int32_t* nbr /*[N][18] visit indices, -1 = missing*/);
/* gradient S^-1-free: g = J^T W r, diag(J^T W J) and y = J^T W J x over parameter ids [sdf N | albedo N | poses 6K | intr 4 | dist 5], visit order */
int i3d_debug_normal_eq(i3d_context* ctx, double* gradient, double* jtj_diag, double* cost);
int i3d_debug_jtj_apply(i3d_context* ctx, const double* x, double* y);
/* the work list of the last assemble (valid after i3d_debug_assemble; launches nothing): visit_index[a] = the visit-order index of work-list entry a, a = 0 .. A-1 — the
 * order in which the row passes walk the voxels (a wave holds 64 consecutive entries).  *count = A; entries are written only when A <= capacity (visit_index may be NULL
 * to ask for the count). */
int i3d_debug_work_list(i3d_context* ctx, int32_t* visit_index /*[capacity]*/, int64_t capacity, int64_t* count);
/* counters of the context since its creation: stream synchronisations of the solver path (assemble + the LM loop).  The trust-region loop of
 * NLSSolver::solve (nls_solver.cpp:296-337) runs on the device; a Gauss-Newton iteration costs a handful of them, not two per LM attempt. */
int i3d_debug_counters(i3d_context* ctx, int64_t* stream_syncs);
/* the damping ladder of the trust-region loop (consecutive LM attempts of NLSSolver::solve, nls_solver.cpp:296-337, whose radii are known in advance are solved
 * together, I3D_LADDER): since the context was created — [0] batches, [1] streams of the stored rows (operator launches of ladder solves), [2] system passes (what
 * the serial loop would have streamed), [3] batches that went out of step (invalid step) and were re-solved, [4] systems solved but never decided (an earlier
 * attempt of their batch was accepted), [5] the batch depth in force (1 = serial loop). */
int i3d_debug_ladder_stats(i3d_context* ctx, int64_t* out6);
/* operator passes of the damping ladder since the context was created, by the number of systems the host held live: out8[n] = passes with n live systems (n = 0 .. 6),
   out8[7] = passes issued as ONE paired launch (4 .. 6 live systems, both groups in one stream of the rows) */
int i3d_debug_ladder_passes(i3d_context* ctx, int64_t* out8);
/* the controller of the trust-region loop alone (tests only): the kernels that start an attempt and decide it (NLSSolver::solve, nls_solver.cpp:296-337, as the device
 * restates it) run on a SCRIPT of attempt outcomes - what the PCG solve, the candidate and the cost pass would have left - through the launches of the product's loop
 * and in its order.  Needs a context, no grid; allocates its own buffers and leaves the context's solver state alone.
 *   plan empty (n_plan = 0): the serial loop.  Otherwise batch sizes 1..6 of the damping ladder, the last one repeated; a record of kind 3 (ladder out of step) is
 *   returned, its slot cleared, and that attempt starts a batch of one, as in the product.
 * records [128]: every record written, in the order read (kind: 0 initial tests | 1 decided attempt | 2 ended before the attempt | 3 not decided).
 * state25: cost, radius, decrease_factor, ngrad, nfree, inv_radius, done, termination, accepted, invalid, attempts, successful, lad_n, lad_radius[6], lad_inv_radius[6].
 * One SETUP per attempt begun (serial) or per system of every batch (ladder), max_setups at most: setup_meta[4] = attempt, system j, batch size (0 = serial), the
 * state's `done` behind the begin kernel; setup_radius / setup_inv_radius: what the begin kernel set for it; setup_blocks [max_setups][G + 36K+41 + G], setup_d2 and
 * setup_minv [max_setups][G + 6K+9 + G], G = I3D_LM_SCRIPT_GUARD floats of NaN either side; what no kernel wrote is NaN (setup_minv: written by the serial loop only). */
#define I3D_LM_SCRIPT_GUARD 64
typedef struct i3d_lm_script_desc {
    double cost, ngrad, nfree, radius0;
    int32_t lm_steps;                        /* 1 .. 62 */
    int32_t K, fix_poses, fix_intr, fix_dist;
    int32_t n_attempts;                      /* >= lm_steps: length of the per-attempt arrays */
    int32_t n_plan, max_setups;
    const double* cdiag;                     /* [6K+9] squared column norms of the camera unknowns */
    const double* tri;                       /* [21K+25] upper triangles of the camera blocks of J^T J */
    const float* tail_c; const float* tail_S;/* [6K+9] the same norms and the Jacobi scaling, as the vector kernels hold them */
    const double* xbr; const double* d2xx; const int32_t* pcg_it; const int32_t* pcg_done;      /* terminal state of each attempt's PCG solve */
    const double* norms2;                    /* [n_attempts][2] |delta|^2, |x|^2 */
    const double* cand_cost; const int32_t* debug_invalid;
    const int32_t* plan;                     /* [n_plan] */
} i3d_lm_script_desc;
typedef struct i3d_lm_record { int32_t seq, final_, accepted, pcg_it, termination, kind; double cost, cand_cost, model_change, rel, radius_after, ngrad, nfree; } i3d_lm_record;
int i3d_debug_lm_script(i3d_context* ctx, const i3d_lm_script_desc* script, i3d_lm_record* records /*[128]*/, int32_t* n_records, double* state25, int32_t* n_setups,
                        int32_t* setup_meta, double* setup_radius, float* setup_inv_radius, float* setup_blocks, float* setup_d2, float* setup_minv);
/* the conservative culling in front of the observation pass (SDFColorization::computeObservation is evaluated per (voxel, keyframe), colorization.cpp:215-315;
 * the device skips (group of 64 voxels, keyframe) pairs no voxel of which can be observed): pairs of the last assemble and how many were skipped.  culled = -1 when
 * culling is off (I3D_NO_CULL=1). */
int i3d_debug_cull_stats(i3d_context* ctx, int64_t* pairs, int64_t* culled);

/* point-set registration (tests only): one pass of the sums at pose6 about the given pivot (world, metres) - the 21 upper-triangle entries of J^T J row by row,
 * the 6 of J^T r, r^2 and the inlier count - and the valid count; desc->iterations is not used.  i3d_debug_register_row_cap lowers the
 * 8192 slab rows a pass may use on this context (0 restores the default), so that a small point set walks more than one point per lane. */
int i3d_debug_register_sums(i3d_context* ctx, const i3d_register_desc* desc, int64_t n, const double* points, const double* pose6, const double* pivot3,
                            double* sums29, int64_t* valid);
int i3d_debug_register_row_cap(i3d_context* ctx, int32_t rows);
/* depth frames on the field (tests only): one pass of the sums of i3d_track_frame_sdf at pose6 (world->camera) about the given pivot (world, metres) - the 29 sums
 * of i3d_debug_register_sums, the 27 of the system weighted when desc->huber_delta > 0 - with the valid and the usable-sample counts; desc->iterations is not
 * used.  i3d_debug_register_row_cap applies to this pass too. */
int i3d_debug_track_sdf_sums(i3d_context* ctx, const i3d_track_sdf_desc* desc, int32_t width, int32_t height, const float* depth,
                             const double* pose6 /* world->camera */, const double* pivot3, double* sums29, int64_t* valid, int64_t* valid_pixels);
/* test only: frames per internal chunk of i3d_track_frames_sdf / i3d_track_keyframes_sdf on this context (<= 0: the default rule) */
int i3d_debug_track_batch_frames(i3d_context* ctx, int32_t frames_per_chunk);
/* the photometric term on the field (tests only): one pass of the combined sums of i3d_track_frame_sdf_rgbd at pose6 about the given pivot - the 27 entries of the
 * combined system, the geometric r^2 and inlier count, then the photometric r^2 and sample count - with the valid count; desc->base.iterations is not used.
 * i3d_debug_register_row_cap applies. */
int i3d_debug_track_sdf_rgbd_sums(i3d_context* ctx, const i3d_track_sdf_rgbd_desc* desc, int32_t width, int32_t height, const float* depth, const float* luminance,
                                  const double* pose6 /* world->camera */, const double* pivot3, double* sums31, int64_t* valid, int64_t* photo_samples);
/* the per-voxel intensity a call of i3d_track_frame_sdf_rgbd would build now: c[N] in visit order, NaN where it is not defined */
int i3d_debug_voxel_intensity(i3d_context* ctx, int32_t use_refined_sdf, double* c);
/* the device stage of i3d_estimate_sh as that call runs it (the same function), handed out before any solve: the subvolume set in the order
 * i3d_estimate_sh reports it, the 10 x 10 Gram block sum w [phi; I][phi; I]^T and the weight sum of every subvolume, and per voxel (visit order) the position of its
 * subvolume in that list, -1 where the voxel is not eligible for the data term.  Any output may be null.  Nothing is solved; the per-voxel SH, the cached subvolumes
 * and what i3d_render_view's shading needs are left as they were.  I3D_SH_SLAB and a communicator act as in i3d_estimate_sh (every rank calls; all get the reduced
 * sums).  Errors as i3d_estimate_sh: I3D_ERR_STATE without a grid, I3D_ERR_INVALID_ARGUMENT for thres_shell <= 0, I3D_ERR_CAPACITY for cap < the subvolume count. */
int i3d_debug_sh_stages(i3d_context* ctx, float subvolume_size, double thres_shell, int32_t cap, int32_t* num_subvolumes, int32_t* sub_index /*[cap][3]*/,
                        double* gram /*[cap][100]*/, double* weight_sum /*[cap]*/, int32_t* voxel_subvolume /*[N]*/);
/* the same two for the fusion volume (tests only): the luminance volume a call of i3d_fusion_track_sdf_rgbd would build now at the n voxel
 * keys given, NaN where the key is not stored or the voxel has weight 0; one pass of the combined sums, as i3d_debug_track_sdf_rgbd_sums */
int i3d_fusion_debug_voxel_luminance(i3d_fusion* f, int64_t n, const int32_t* keys /*[n][3]*/, double* c /*[n]*/);
int i3d_fusion_debug_track_sdf_rgbd_sums(i3d_fusion* f, const i3d_track_sdf_rgbd_desc* desc, int32_t width, int32_t height, const float* depth,
                                         const float* luminance, const double* pose6 /* world->camera */, const double* pivot3, double* sums31, int64_t* valid,
                                         int64_t* photo_samples);
/* tests only, by key lookup; both leave the table untouched (the second uploads the frame into the handle's frame buffers, as
 * i3d_fusion_integrate does): the live table's state at n voxel keys - found 0 / 1, sdf, weight, colour R,G,B, and the ordinal of
 * the frame that first inserted the voxel (-1 where the key is not stored) ... */
int i3d_fusion_debug_voxels(i3d_fusion* f, int64_t n, const int32_t* keys /*[n][3]*/, uint8_t* found, float* sdf, float* weight, uint8_t* color /*[n][3]*/,
                            int64_t* first_frame);
/* ... and the contribution the given frame makes to those voxels, whether stored or not (the function integrate, deintegrate and reintegrate share): on = the
 * gates pass, the sample d - z, the weight, and the colour sample R,G,B where has_color */
int i3d_fusion_debug_frame_samples(i3d_fusion* f, int32_t depth_w, int32_t depth_h, const float* depth_intr4, int32_t color_w, int32_t color_h, const float* color_intr4,
                                   const float* depth, const uint8_t* bgr, const float* pose_cam_to_world16, int32_t erode_window, int64_t n,
                                   const int32_t* keys /*[n][3]*/, uint8_t* on, float* sample, float* wu, uint8_t* has_color, uint8_t* rgb /*[n][3]*/);
/* tests only: overwrite sdf, weight and colour of the voxels that ARE stored at the n distinct keys (nothing is inserted); found[i] = 0 and
 * nothing written where the key is not stored; drops the cached brick bitmap; before or after finish */
int i3d_fusion_debug_poke_voxels(i3d_fusion* f, int64_t n, const int32_t* keys /*[n][3]*/, const float* sdf, const float* weight, const uint8_t* color /*[n][3]*/,
                                 uint8_t* found);
/* tests only: the list of src's samples in its order - *count its length, the first min(count, capacity) entries written - and one pass of
 * the sums at pose6 about pivot3 over the first `limit` entries of the list (0: all) with at most row_cap slab rows (0: 8192) */
int i3d_fusion_debug_register_volume_selection(i3d_fusion* src, const i3d_register_volume_desc* desc, int64_t capacity, int32_t* keys /*[capacity][3]*/,
                                               float* sdf /*[capacity]*/, int64_t* count);
int i3d_fusion_debug_register_volume_sums(i3d_fusion* f, i3d_fusion* src, const i3d_register_volume_desc* desc, const double* pose6, const double* pivot3,
                                          int64_t limit, int32_t row_cap, double* sums29, int64_t* valid, int64_t* selected);
/* tests only: the keys of the stored voxels, weight-0 ones included, in ascending first-insertion rank - the sequence the replay of finish
 * and snapshot starts from.  *count is always written; capacity < count is I3D_ERR_CAPACITY with no keys written.  Leaves the table untouched. */
int i3d_fusion_debug_insertion_order(i3d_fusion* f, uint64_t capacity, int32_t* keys /*[capacity][3]*/, uint64_t* count);

#ifdef __cplusplus
}
#endif
#endif
