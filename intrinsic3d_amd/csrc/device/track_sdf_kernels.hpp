// Registration of depth frames on the stored field, no ray cast (track_sdf_kernels.hip; i3d_track_frame_sdf, its batch, rgbd and fusion forms).  The definition
// the kernels implement is DESIGN.md section 19: the samples of the depth image are back-projected inside the sums kernel and registered as the points of section
// 18.  The Gauss-Newton step is k_track_solve on a TrackState (track_kernels.hpp); the block / lane / P layout is that of register_kernels.hpp over the samples.
// There is one form of every launch, over the frames of a TrackSdfBatch: the single-frame entry points pass one frame.
#pragma once
#include "register_kernels.hpp"

namespace i3d {

constexpr int TRACK_SDF_COL_USABLE = 30;          // slab column of the usable-sample count (29 is the valid count, as in k_register); the photometric passes
                                                  // keep sum r_p^2 there (TRACK_COL_PHOTO_SQ) and take the count from the pivot pass
constexpr int TRACK_SDF_MEAN_COL_USABLE = 4;      // pivot pass: column of the usable-sample count (every sample whose depth is usable, counted or not)

struct TrackSdfParams {
    PinholeCam cam;                                 // level 0, the whole image (w, h)
    int stride, ws;                               // sample i is pixel ((i % ws) * stride, (i / ws) * stride)
    long long n;                                  // ws * hs samples
    int per_lane;                                 // P, as RegisterParams
    float min_depth, max_depth;                   // <= 0: open
    double max_distance;                          // gate on |f|
    double huber_delta;                           // k of the Huber weight; read by the HUBER instantiations only
};

// the frames of a pass, all of one size and one camera: device arrays indexed by the frame (blockIdx.y).  A single frame is frames == 1
struct TrackSdfBatch {
    const float* const* depth;                    // [frames] device pointers to the frames' images, [h][w] each
    const float* const* lum;                      // [frames] the frames' luminance images likewise; read by the passes with a photometric term only
    const TrackState* state;                      // [frames]
    const double* pivot;                          // [frames][3]: a state's t is t - c, a point is placed at x' = R p + t' and looked up at x' + c
    double* slab;                                 // [frames][register_rows(n, per_lane)][TRACK_COLS], a frame's rows fully overwritten by a pass that runs on it
    int frames;                                   // <= 65535 (gridDim.y)
};

// The photometric term on the field (i3d_track_frame_sdf_rgbd): the per-voxel intensity c = albedo x SH shading at the voxel's normal,
// one fp64 value per stored voxel in device order, a quiet NaN where it is not defined.  Filled by launch_voxel_intensity; the sums kernel samples it over the
// cell it already holds, as a second field
struct TrackSdfPhoto {
    const double* vol;                            // [N]; null: no photometric block runs (photo weight 0)
    double wg2, wp2;                              // squared weights of the two terms
    double max_residual;                          // gate on |r_p|; <= 0: open
};

// the pivot means of every frame at the pose R, t of its state (the start pose, not yet about a pivot): columns 0..2 the sum of the back-projected points of the
// usable samples that count (R p + t within the coordinate range of the point query), column 3 their number, column 4 the number of usable samples, the rest 0
void launch_track_sdf_mean(hipStream_t st, const TrackSdfParams& p, const TrackSdfBatch& b, double vs);
// one pass of every frame at the pose of its state about its pivot; check_done: the workgroups of a frame whose state is done return at once.
// photo == null: the 29 sums of TRACK_SUMS over the inliers (the 27 weighted when huber_delta > 0), column 29 the valid count, column 30 the usable count.
// photo != null: the combined system - the 27 entries are wg2 (omega) J_g J_g^T + wp2 J_p J_p^T (J^T r likewise), columns 27 / 28 the geometric r^2 and count,
// 29 the valid count, 30 / 31 the photometric r^2 and sample count.  Over the fusion table the corners of a cell are table slots, so photo->vol is the volume of
// launch_fusion_voxel_luminance
void launch_track_sdf(hipStream_t st, const RenderGrid& g, const TrackSdfParams& p, const TrackSdfPhoto* photo, const TrackSdfBatch& b, int check_done);
void launch_track_sdf(hipStream_t st, const FusionRenderGrid& g, const TrackSdfParams& p, const TrackSdfPhoto* photo, const TrackSdfBatch& b, int check_done);

// out[s] for every stored voxel s of g (g.sdf the chosen field, g.alb, g.sh); one lane per voxel
void launch_voxel_intensity(hipStream_t st, const RenderGrid& g, double* out);
// The same term on the fusion volume (i3d_fusion_track_sdf_rgbd): the volume is the luminance of the fused colour, one fp64 value per table
// slot, a quiet NaN where the slot is empty or has weight 0.  out: [t.mask + 1]; one lane per slot
void launch_fusion_voxel_luminance(hipStream_t st, const FusionTable& t, double* out);
// tests only: out[i] = vol[slot of keys[i]] for n voxel keys [n][3], a quiet NaN when the key is not stored
void launch_fusion_luminance_lookup(hipStream_t st, const FusionTable& t, const double* vol, long long n, const int* keys, double* out);

}  // namespace i3d
