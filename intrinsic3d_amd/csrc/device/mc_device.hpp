// The marching-cubes arithmetic both mesh extractions run (mesh_kernels.hip on the resident grid, fusion_mesh_kernels.hip on the fusion table): ONE definition of the
// edge numbering and of the interpolation, so that the two produce the same bits for the same cell.  Both files are compiled with -ffp-contract=off.
// Cube corners use the reference's numbering (corner 0 = (x+1,y+1,z), 1 = (x+1,y,z), 2 = (x,y,z), 3 = (x,y+1,z), 4..7 the same at z+1); edge e joins corners
// mc_ea(e) -> mc_eb(e) in that direction, which fixes the interpolation formula's operand order.
#pragma once
#include <hip/hip_runtime.h>

namespace i3d {

__device__ inline int mc_ea(int e) { constexpr int EA[12] = {0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3}; return EA[e]; }
__device__ inline int mc_eb(int e) { constexpr int EB[12] = {1, 2, 3, 0, 5, 6, 7, 4, 4, 5, 6, 7}; return EB[e]; }

// MarchingCubes::interpolate (marching_cubes.cpp:297-309) on one component
__device__ inline float mc_lerp(float t0, float t1, float v0, float v1) {
    if (fabsf(0.0f - t0) < 0.00001f) return v0;
    if (fabsf(0.0f - t1) < 0.00001f) return v1;
    if (fabsf(t0 - t1) < 0.00001f) return v0;
    float mu = (0.0f - t0) / (t1 - t0);
    mu = fmaxf(fminf(mu, 1.0f), 0.0f);
    return v0 + mu * (v1 - v0);
}

}  // namespace i3d
