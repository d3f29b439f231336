// The one statement of the registration pass of DESIGN.md section 18 (and of section 28, which is section 18's geometry, sums and step over another point source):
//   register_mean_body<Src>     the pivot: per workgroup the sum and the number of the points that count, one slab row
//   register_pass_body<G, Src>  one lane per point (P points per lane when the slab would exceed 8192 rows), 256 lanes per workgroup: the point placed by the pose
//                               of the device state, the trilinear cell of cell_device.hpp there, the residual and its Jacobian in fp64, the 29 sums + the valid
//                               count summed over the wave by the reduce-scatter butterfly of k_track_assoc, over the workgroup through LDS in wave order, one slab
//                               row per workgroup
// Src is the point source, passed by value:
//   point(i, p)      the point of entry i
//   counts(p)        whether the point can count at all towards the pivot (raw points: three finite coordinates; list entries: always)
//   skip(g, x)       a test that may drop the placed point x before the cell is looked up; decides nothing cell_of_point would decide otherwise
//   residual(f, i)   the residual of entry i from the field value f at the placed point
// The __global__ wrappers, their launchers and the translation units' flags stay with register_kernels.hip and register_volume_kernels.hip: both are compiled with
// -ffp-contract=off, and their numpy statements (tests/register_twin.py, tests/register_volume_twin.py) evaluate these very fp64 expressions in this order.
#pragma once
#include "register_kernels.hpp"
#include "point_cell_device.hpp"
#include "slab_device.hpp"

namespace i3d {

struct MeanParams { long long n; int per_lane; double R[9], t[3], vs; };

inline MeanParams mean_params(long long n, int per_lane, const double* R0, const double* t0, double vs) {
    MeanParams prm; prm.n = n; prm.per_lane = per_lane; prm.vs = vs;
    for (int i = 0; i < 9; ++i) prm.R[i] = R0[i];
    for (int a = 0; a < 3; ++a) prm.t[a] = t0[a];
    return prm;
}

template <class Src>
__device__ inline void register_mean_body(const MeanParams& prm, const Src& src, double* __restrict__ slab) {
    __shared__ double part[REGISTER_BLOCK / 64][TRACK_COLS];
    double s[TRACK_COLS];
#pragma unroll
    for (int k = 0; k < TRACK_COLS; ++k) s[k] = 0.0;
    const long long base = (long long)blockIdx.x * REGISTER_BLOCK * prm.per_lane + threadIdx.x;
    for (int j = 0; j < prm.per_lane; ++j) {
        const long long i = base + (long long)j * REGISTER_BLOCK;
        if (i < prm.n) {                             // tail lanes fall through to the shuffles with zeros
            double p[3]; src.point(i, p);
            bool ok = src.counts(p);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double x = ((prm.R[3 * a] * p[0] + prm.R[3 * a + 1] * p[1]) + prm.R[3 * a + 2] * p[2]) + prm.t[a];
                ok = ok && isfinite(x) && fabs(x / prm.vs) < QUERY_MAX_COORD;
            }
            if (ok) { s[0] = s[0] + p[0]; s[1] = s[1] + p[1]; s[2] = s[2] + p[2]; s[3] = s[3] + 1.0; }
        }
    }
    slab_row(s, part, slab);
}

template <class G, class Src>
__device__ inline void register_pass_body(const G& g, const RegisterParams& prm, const Src& src, const TrackState* __restrict__ st, int check_done,
                                          double* __restrict__ slab) {
    __shared__ double part[REGISTER_BLOCK / 64][TRACK_COLS];
    if (check_done && st->done) return;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = st->R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = st->t[i];
    const double vs = g.vs;
    double s[TRACK_COLS];
#pragma unroll
    for (int k = 0; k < TRACK_COLS; ++k) s[k] = 0.0;
    const long long base = (long long)blockIdx.x * REGISTER_BLOCK * prm.per_lane + threadIdx.x;
    for (int j = 0; j < prm.per_lane; ++j) {
        const long long i = base + (long long)j * REGISTER_BLOCK;
        if (i >= prm.n) break;                       // tail lanes fall through to the shuffles with zeros
        double p[3]; src.point(i, p);
        double xp[3], x[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            xp[a] = ((R[3 * a] * p[0] + R[3 * a + 1] * p[1]) + R[3 * a + 2] * p[2]) + t[a];
            x[a] = xp[a] + prm.c[a];
        }
        if (src.skip(g, x)) continue;
        CellCache cc; cell_cache_reset(cc);
        if (!cell_of_point(g, cc, x)) continue;
        s[29] = s[29] + 1.0;
        const double r = src.residual(field(cc), i);
        if (!(fabs(r) <= prm.max_distance)) continue;
        double gr[3]; cell_gradient(cc, gr);
        const double d0 = gr[0] / vs, d1 = gr[1] / vs, d2 = gr[2] / vs;
        const double J[6] = {xp[1] * d2 - xp[2] * d1, xp[2] * d0 - xp[0] * d2, xp[0] * d1 - xp[1] * d0, d0, d1, d2};
        add_normal_row(s, J, r, 27, [](double x) { return x; });
    }
    slab_row(s, part, slab);
}

}  // namespace i3d
