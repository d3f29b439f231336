// Rigid alignment of a point set to the stored field (register_kernels.hip, i3d_register_points / i3d_fusion_register_points).  The definition the kernels
// implement is DESIGN.md section 18; the Gauss-Newton step is k_track_solve on a TrackState (track_kernels.hpp), its slab rows are written here.
#pragma once
#include "render_kernels.hpp"
#include "track_kernels.hpp"

namespace i3d {

constexpr int REGISTER_BLOCK = TRACK_BLOCK;       // lanes per workgroup; a workgroup owns REGISTER_BLOCK * per_lane consecutive points
constexpr int REGISTER_MAX_ROWS = 8192;           // slab rows of a pass at most

struct RegisterParams {
    long long n;
    int per_lane;                                 // P: points a lane walks, ascending (point = block * 256 * P + j * 256 + lane, j = 0 .. P - 1)
    double max_distance;                          // gate on |f|
    double c[3];                                  // the pivot: the state's t is t - c, a point is placed at x' = R p + t' and looked up at x' + c
};

// P: the smallest power of two with ceil(n / (256 P)) <= row_cap
inline int register_per_lane(long long n, int row_cap) {
    long long p = 1;
    while ((n + REGISTER_BLOCK * p - 1) / (REGISTER_BLOCK * p) > (long long)row_cap) p *= 2;
    return (int)p;
}
inline int register_rows(long long n, int per_lane) { return (int)((n + (long long)REGISTER_BLOCK * per_lane - 1) / ((long long)REGISTER_BLOCK * per_lane)); }

// slab: [register_rows][TRACK_COLS], fully overwritten by a pass that runs.  The grids' brick bitmaps are not read.
// the pivot mean: columns 0..2 the sum of the points that count (three finite coordinates, R0 p + t0 within the coordinate range of the point query), column 3
// their number, the rest 0
void launch_register_mean(hipStream_t st, long long n, int per_lane, const double* points, const double* R0 /*[9] host*/, const double* t0 /*[3] host*/, double vs,
                          double* slab);
// one pass at the pose of *state: the 29 sums of TRACK_SUMS over the inliers, column 29 the valid count; check_done: return at once when state->done
void launch_register(hipStream_t st, const RenderGrid& g, const RegisterParams& p, const double* points, const TrackState* state, int check_done, double* slab);
void launch_register(hipStream_t st, const FusionRenderGrid& g, const RegisterParams& p, const double* points, const TrackState* state, int check_done, double* slab);

}  // namespace i3d
