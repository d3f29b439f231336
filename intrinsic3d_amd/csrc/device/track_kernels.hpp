// Registration of a depth frame against the resident model (track_kernels.hip, i3d_track_frame).  The definition the kernels implement is DESIGN.md section 14;
// the photometric term of i3d_track_frame_rgbd is section 16.
#pragma once
#include "kernels.hpp"
#include "camera_device.hpp"

namespace i3d {

constexpr int TRACK_SUMS = 29;                    // 21 upper-triangle J^T J (row by row) | 6 J^T r | r^2 | inlier count
constexpr int TRACK_COLS = 32;                    // a slab row: the 29 sums, the valid-pixel count, then sum r_p^2 and the photometric sample count (zero without a photometric term)
constexpr int TRACK_COL_PHOTO_SQ = 30, TRACK_COL_PHOTO_N = 31;
constexpr int TRACK_BLOCK = 256;                  // pixels per workgroup of k_track_assoc = rows of the slab per 256 pixels
constexpr int TRACK_MIN_INLIERS = 64;             // fewer inliers (photometric samples when the geometric weight is 0): status 2

struct TrackRef {                                 // the pose of the level's ray cast
    double R[9];                                  // world -> camera rotation, row-major
    double t[3];                                  // world -> camera translation
    double eye[3];                                // camera centre in the world frame
};

struct TrackState {                               // device-resident state of one level's Gauss-Newton loop; the host writes it before the level and reads it after
    double R[9], t[3];                            // current estimate, camera -> world (p = R v + t)
    double sums[TRACK_COLS];                      // totals of the last pass
    double rms_first;                             // RMS of the level's first association
    double min_pivot_ratio;                       // of the last factorised system
    int done, iters, status, first;               // done: the remaining launched passes of the level return at once
    double rms_first_photo;                       // rms_first of the photometric residuals (0 without them)
};

void launch_track_points(hipStream_t st, const PinholeCam& cam, const float* depth, float min_depth, float max_depth, float* vtx, float* nrm);
int track_assoc_rows(int w, int h);               // slab rows (workgroups) of one association pass
struct TrackPhoto {                               // the photometric term of an association pass
    const float* lum;                             // frame luminance of the level
    const float* mintensity;                      // model intensity plane of the level's ray cast; null: no photometric sample is taken (photo weight 0)
    double wg2, wp2;                              // squared weights of the two terms
    double max_distance;                          // a bilinear tap's model depth may differ from the associated pixel's by at most this
    double max_residual;                          // gate on |r_p|; <= 0: open
};
// cam: the camera of the level (the frame's and the ray cast's).  photo == null: the 29 sums over the inliers and the valid-pixel count, columns 30 / 31 zero.
// photo != null: the 27 entries are wg2 J_g J_g^T + wp2 J_p J_p^T (and J^T r likewise); columns 27 / 28 the geometric r^2 and count, 30 / 31 the photometric ones
void launch_track_assoc(hipStream_t st, const PinholeCam& cam, const TrackRef& ref, const float* vtx, const float* nrm, const float* mdepth, const float* mnormal,
                        const TrackPhoto* photo, double max_distance, double min_normal_dot, const TrackState* state, int check_done, double* slab);
// `frames` independent loops in one launch: workgroup f works on states[f] and on the rows of slab + f * rows * TRACK_COLS.  mode 0: one Gauss-Newton step
// (skipped when done); mode 1: the totals only, into the state's sums.  count_col: the column whose total must reach TRACK_MIN_INLIERS (28: geometric inliers;
// TRACK_COL_PHOTO_N when the geometric weight is 0)
void launch_track_solve(hipStream_t st, TrackState* states, const double* slab, int frames, int rows, int mode, int count_col, double stop_rotation,
                        double stop_translation);

}  // namespace i3d
