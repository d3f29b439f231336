// The trilinear cell of the stored field in fp64: one definition for every kernel that samples it (the ray cast of render_kernels.hip, the point query of
// query_kernels.hip).  A cell is valid iff its 8 corners are stored with weight != 0 (the marching-cubes rule, mesh_kernels.hip cell_config); corner
// i = base + (i & 1, (i >> 1) & 1, i >> 2).  The files that include this are compiled with -ffp-contract=off: the numpy statements of their definitions
// (tests/render_twin.py, tests/query_twin.py) evaluate the same expressions in the same order.
#pragma once
#include "render_kernels.hpp"
#include "voxel_hash.hpp"
#include "fusion_hash.hpp"
#include <climits>

namespace i3d {

// the cell based at (bx, by, bz) of the context's grid
__device__ inline bool load_cell(const RenderGrid& g, int bx, int by, int bz, int (&c)[8], double (&v)[8]) {
    const int s = hash_find(g.t, bx, by, bz);
    if (s < 0) return false;
    const size_t N = (size_t)g.N;
    c[0] = s; c[1] = g.nbr[NB_PX * N + s]; c[2] = g.nbr[NB_PY * N + s]; c[3] = g.nbr[NB_PXY * N + s];
    c[4] = g.nbr[NB_PZ * N + s]; c[5] = g.nbr[NB_PXZ * N + s]; c[6] = g.nbr[NB_PYZ * N + s];
    if (c[1] < 0 || c[2] < 0 || c[3] < 0 || c[4] < 0 || c[5] < 0 || c[6] < 0) return false;
    c[7] = hash_find(g.t, bx + 1, by + 1, bz + 1);
    if (c[7] < 0) return false;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) ok &= g.weight[c[i]] != 0.0f;
    if (!ok) return false;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = g.sdf[c[i]];
    return true;
}

// the same cell of the fusion volume: each corner probed in the table, valid iff all 8 are stored with weight != 0, the float sdf widened to fp64; `c` gets the
// corners' table slots (a table has at most 2^31 of them), which only the photometric sums read.  A base whose (+1, +1, +1) corner has no packed key cannot have 8 stored corners.
__device__ inline bool load_cell(const FusionRenderGrid& g, int bx, int by, int bz, int (&c)[8], double (&v)[8]) {
    constexpr int K = FUSION_COORD_OFFSET;
    if (bx < -K || by < -K || bz < -K || bx >= K - 1 || by >= K - 1 || bz >= K - 1) return false;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const long long s = fusion_hash::find_slot(g.t, fusion_hash::pack_key(bx + (i & 1), by + ((i >> 1) & 1), bz + (i >> 2)));
        if (s < 0 || g.t.weight[s] == 0.0f) return false;
        c[i] = (int)s;
        v[i] = (double)g.t.sdf[s];
    }
    return true;
}

// a one-cell cache: position in voxel units q, base b = floor(q), frac = q - base
struct CellCache {
    int b[3]; bool valid; int c[8]; double v[8];
    double f[3];                                  // fractional position of the last evaluation
};

__device__ inline void cell_cache_reset(CellCache& cc) { cc.b[0] = INT_MIN; cc.b[1] = INT_MIN; cc.b[2] = INT_MIN; cc.valid = false; }

template <class G>
__device__ inline bool cell_at(const G& g, CellCache& cc, const double (&q)[3], const int (&b)[3]) {
    if (b[0] != cc.b[0] || b[1] != cc.b[1] || b[2] != cc.b[2]) {
        cc.b[0] = b[0]; cc.b[1] = b[1]; cc.b[2] = b[2];
        cc.valid = load_cell(g, b[0], b[1], b[2], cc.c, cc.v);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) cc.f[a] = q[a] - (double)b[a];
    return cc.valid;
}

__device__ inline void tri_weights(const double (&f)[3], double (&w)[8]) {
    const double gx = 1.0 - f[0], gy = 1.0 - f[1], gz = 1.0 - f[2];
    w[0] = gx * gy * gz; w[1] = f[0] * gy * gz; w[2] = gx * f[1] * gz; w[3] = f[0] * f[1] * gz;
    w[4] = gx * gy * f[2]; w[5] = f[0] * gy * f[2]; w[6] = gx * f[1] * f[2]; w[7] = f[0] * f[1] * f[2];
}

__device__ inline double tri_sum(const double (&w)[8], const double (&v)[8]) {
    double s = w[0] * v[0];
#pragma unroll
    for (int i = 1; i < 8; ++i) s = s + w[i] * v[i];
    return s;
}

__device__ inline double field(const CellCache& cc) { double w[8]; tri_weights(cc.f, w); return tri_sum(w, cc.v); }

// gradient of the interpolant per voxel at the cache's fractional position
__device__ inline void cell_gradient(const CellCache& cc, double (&g)[3]) {
    const double fx = cc.f[0], fy = cc.f[1], fz = cc.f[2], gx = 1.0 - fx, gy = 1.0 - fy, gz = 1.0 - fz;
    const double* vv = cc.v;
    g[0] = (((vv[1] - vv[0]) * gy * gz + (vv[3] - vv[2]) * fy * gz) + (vv[5] - vv[4]) * gy * fz) + (vv[7] - vv[6]) * fy * fz;
    g[1] = (((vv[2] - vv[0]) * gx * gz + (vv[3] - vv[1]) * fx * gz) + (vv[6] - vv[4]) * gx * fz) + (vv[7] - vv[5]) * fx * fz;
    g[2] = (((vv[4] - vv[0]) * gx * gy + (vv[5] - vv[1]) * fx * gy) + (vv[6] - vv[2]) * gx * fy) + (vv[7] - vv[3]) * fx * fy;
}

}  // namespace i3d
