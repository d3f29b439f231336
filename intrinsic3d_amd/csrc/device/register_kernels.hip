// Rigid alignment of a point set to the stored field (i3d_register_points / i3d_fusion_register_points; the definition is DESIGN.md section 18).
//   k_register_mean  the pivot: per workgroup the sum and the number of the points that count, one slab row
//   k_register<G>    one lane per point (P points per lane when the slab would exceed 8192 rows), 256 lanes per workgroup: the point placed by the pose of the
//                    device state, the trilinear cell of cell_device.hpp there, the residual f and its Jacobian in fp64, the 29 sums + the valid count summed over
//                    the wave by the reduce-scatter butterfly of k_track_assoc, over the workgroup through LDS in wave order, one slab row per workgroup.
//                    G = RenderGrid (the context's grid) or FusionRenderGrid (the fusion table as it stands)
// The rows are totalled and the 6x6 step taken by k_track_solve (track_kernels.hip).  No floating-point atomics: every sum has an order that depends on n alone.
// Compiled with -ffp-contract=off: the numpy statement of the definition (tests/register_twin.py) evaluates the same fp64 expressions in the same order.
#include "register_kernels.hpp"
#include "point_cell_device.hpp"
#include "slab_device.hpp"

namespace i3d {
namespace {

struct MeanParams { long long n; int per_lane; double R[9], t[3], vs; };

__global__ void __launch_bounds__(REGISTER_BLOCK) k_register_mean(MeanParams prm, const double* __restrict__ points, double* __restrict__ slab) {
    __shared__ double part[REGISTER_BLOCK / 64][TRACK_COLS];
    double s[TRACK_COLS];
#pragma unroll
    for (int k = 0; k < TRACK_COLS; ++k) s[k] = 0.0;
    const long long base = (long long)blockIdx.x * REGISTER_BLOCK * prm.per_lane + threadIdx.x;
    for (int j = 0; j < prm.per_lane; ++j) {
        const long long i = base + (long long)j * REGISTER_BLOCK;
        if (i < prm.n) {                             // tail lanes fall through to the shuffles with zeros
            const double p[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
            bool ok = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
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

template <class G>
__global__ void __launch_bounds__(REGISTER_BLOCK) k_register(G g, RegisterParams prm, const double* __restrict__ points, const TrackState* __restrict__ st,
                                                             int check_done, double* __restrict__ slab) {
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
        const double p0 = points[3 * i], p1 = points[3 * i + 1], p2 = points[3 * i + 2];
        double xp[3], x[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            xp[a] = ((R[3 * a] * p0 + R[3 * a + 1] * p1) + R[3 * a + 2] * p2) + t[a];
            x[a] = xp[a] + prm.c[a];
        }
        CellCache cc; cell_cache_reset(cc);
        if (!cell_of_point(g, cc, x)) continue;
        s[29] = s[29] + 1.0;
        const double r = field(cc);
        if (!(fabs(r) <= prm.max_distance)) continue;
        double gr[3]; cell_gradient(cc, gr);
        const double d0 = gr[0] / vs, d1 = gr[1] / vs, d2 = gr[2] / vs;
        const double J[6] = {xp[1] * d2 - xp[2] * d1, xp[2] * d0 - xp[0] * d2, xp[0] * d1 - xp[1] * d0, d0, d1, d2};
        add_normal_row(s, J, r, 27, [](double x) { return x; });
    }
    slab_row(s, part, slab);
}

template <class G>
void launch(hipStream_t st, const G& g, const RegisterParams& p, const double* points, const TrackState* state, int check_done, double* slab) {
    const int rows = register_rows(p.n, p.per_lane);
    if (rows > 0) k_register<G><<<rows, REGISTER_BLOCK, 0, st>>>(g, p, points, state, check_done, slab);
}

}  // namespace

void launch_register_mean(hipStream_t st, long long n, int per_lane, const double* points, const double* R0, const double* t0, double vs, double* slab) {
    MeanParams prm; prm.n = n; prm.per_lane = per_lane; prm.vs = vs;
    for (int i = 0; i < 9; ++i) prm.R[i] = R0[i];
    for (int a = 0; a < 3; ++a) prm.t[a] = t0[a];
    const int rows = register_rows(n, per_lane);
    if (rows > 0) k_register_mean<<<rows, REGISTER_BLOCK, 0, st>>>(prm, points, slab);
}
void launch_register(hipStream_t st, const RenderGrid& g, const RegisterParams& p, const double* points, const TrackState* state, int check_done, double* slab) {
    launch(st, g, p, points, state, check_done, slab);
}
void launch_register(hipStream_t st, const FusionRenderGrid& g, const RegisterParams& p, const double* points, const TrackState* state, int check_done, double* slab) {
    launch(st, g, p, points, state, check_done, slab);
}

}  // namespace i3d
