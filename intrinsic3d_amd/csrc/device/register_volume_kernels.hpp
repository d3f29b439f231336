// Alignment of one fusion volume to another on the stored fields (register_volume_kernels.hip, i3d_fusion_register_volume).  The definition the kernels implement
// is DESIGN.md section 28; geometry, sums and step are section 18's (register_kernels.hpp), the Gauss-Newton step is k_track_solve on a TrackState.
#pragma once
#include "register_kernels.hpp"
#include "fusion_kernels.hpp"

namespace i3d {

// the sorted list of src's selected slots (slot_list.hpp's SlotBand): the payload of an entry is the bits of the sdf stored there
struct VolumeList {                               // ascending packed key; the point of an entry is (double)k[a] * vs
    const unsigned long long* keys; const float* sdf; long long n; double vs;
};

// slab: [register_rows][TRACK_COLS], fully overwritten by a pass that runs; P and the rows as register_per_lane / register_rows over list.n
// the pivot mean over the list: columns 0..2 the sum of the points whose placed position R0 p + t0 is finite and within |x / vs_f| < 2^20, column 3 their number
void launch_register_volume_mean(hipStream_t st, const VolumeList& list, int per_lane, const double* R0 /*[9] host*/, const double* t0 /*[3] host*/, double vs_f,
                                 double* slab);
// one pass at the pose of *state: r = f(R p + t) - s over the list; the 29 sums of TRACK_SUMS over the inliers, column 29 the valid count; p.n = list.n
void launch_register_volume(hipStream_t st, const FusionRenderGrid& g, const RegisterParams& p, const VolumeList& list, const TrackState* state, int check_done,
                            double* slab);

}  // namespace i3d
