// The slab row of a workgroup of 256 lanes that each hold TRACK_COLS fp64 values: one definition for every kernel that feeds k_track_solve.  Fixed order, no
// atomics.
#pragma once
#include "track_kernels.hpp"

namespace i3d {

// wave sum of 32 values by reduce-scatter: at the step of width o a lane keeps the half of its values selected by its lane bit o and adds the partner's copy
// of that half (16 + 8 + 4 + 2 + 1 shuffles, then one for the last pair).  Afterwards lane L holds the total of value (L >> 1) & 31.
__device__ inline double wave_sum32(double (&s)[TRACK_COLS], int lane) {
    double h16[16], h8[8], h4[4], h2[2];
    {
        const bool hi = lane & 32;
#pragma unroll
        for (int i = 0; i < 16; ++i) { const double keep = hi ? s[16 + i] : s[i], give = hi ? s[i] : s[16 + i]; h16[i] = keep + __shfl_xor(give, 32); }
    }
    {
        const bool hi = lane & 16;
#pragma unroll
        for (int i = 0; i < 8; ++i) { const double keep = hi ? h16[8 + i] : h16[i], give = hi ? h16[i] : h16[8 + i]; h8[i] = keep + __shfl_xor(give, 16); }
    }
    {
        const bool hi = lane & 8;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const double keep = hi ? h8[4 + i] : h8[i], give = hi ? h8[i] : h8[4 + i]; h4[i] = keep + __shfl_xor(give, 8); }
    }
    {
        const bool hi = lane & 4;
#pragma unroll
        for (int i = 0; i < 2; ++i) { const double keep = hi ? h4[2 + i] : h4[i], give = hi ? h4[i] : h4[2 + i]; h2[i] = keep + __shfl_xor(give, 4); }
    }
    const bool hi = lane & 2;
    const double keep = hi ? h2[1] : h2[0], give = hi ? h2[0] : h2[1];
    const double h1 = keep + __shfl_xor(give, 2);
    const double other = __shfl_xor(h1, 1);                         // every lane takes part: a shuffle inside a branch would read inactive lanes
    const double lo = (lane & 1) ? other : h1, up = (lane & 1) ? h1 : other;
    return lo + up;                                                // both lanes of the pair: (even lane's part) + (odd lane's part)
}

// the workgroup's row of the slab from every lane's 32 values: the wave butterfly, then the four waves through LDS in wave order
__device__ inline void slab_row(double (&s)[TRACK_COLS], double (&part)[TRACK_BLOCK / 64][TRACK_COLS], double* __restrict__ slab) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double w = wave_sum32(s, lane);
    if ((lane & 1) == 0) part[wave][(lane >> 1) & 31] = w;
    __syncthreads();
    if (threadIdx.x < TRACK_COLS) {
        const int k = threadIdx.x;
        slab[(size_t)blockIdx.x * TRACK_COLS + k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
    }
}

}  // namespace i3d
