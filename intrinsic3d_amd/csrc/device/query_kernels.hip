// The stored field at arbitrary world points (i3d_query_points / i3d_fusion_query_points; the definition is DESIGN.md section 17).
//   k_query<G>       one lane per point, 256 per workgroup: the trilinear cell of cell_device.hpp at the point (value, gradient, albedo), then the Newton walk along
//                    the gradient onto the zero level set; the error figures summed over the wave by a butterfly of shuffles, over the workgroup through LDS in wave
//                    order, one row per workgroup.  G = RenderGrid (the context's grid) or FusionRenderGrid (the fusion table as it stands: no albedo)
//   k_query_reduce   one workgroup: the rows added in a fixed order (lane t: rows t, t + 256, ... ascending; then the 256 partials ascending)
// No floating-point atomics anywhere: the stats of a call are a function of its input alone.  Positions and values in fp64; compiled with -ffp-contract=off:
// the numpy statement of the definition (tests/query_twin.py) evaluates the same expressions in the same order.
#include "query_kernels.hpp"
#include "point_cell_device.hpp"      // cell_of_point
#include <type_traits>

namespace i3d {
namespace {

constexpr int WAVES = QUERY_BLOCK / 64;
constexpr int NSUM = 4, NMAX = 2, NCNT = 3;      // columns of a row: sums | maxima | counts

template <class G>
__global__ void __launch_bounds__(QUERY_BLOCK) k_query(G g, QueryParams prm, const double* __restrict__ points, QueryOut out, QueryRow* __restrict__ rows) {
    constexpr bool ATTRIBUTES = std::is_same<G, RenderGrid>::value;     // albedo exists in the context's grid only
    __shared__ double part_d[WAVES][NSUM + NMAX];
    __shared__ long long part_c[WAVES][NCNT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long i = (long long)blockIdx.x * QUERY_BLOCK + threadIdx.x;
    unsigned char status = 0;
    double f0 = 0.0, dist = 0.0, foot[3] = {0.0, 0.0, 0.0};
    float o_n[3] = {0.0f, 0.0f, 0.0f}, o_alb = 0.0f;
    long long steps = 0;
    if (i < prm.n) {                                 // tail lanes fall through to the shuffles with zero contributions
        const double vs = g.vs;
        const double p0[3] = {points[3 * i], points[3 * i + 1], points[3 * i + 2]};
        CellCache cc; cell_cache_reset(cc);
        if (cell_of_point(g, cc, p0)) {
            status = 1;
            double f = field(cc);
            double gr[3]; cell_gradient(cc, gr);
            double nl = sqrt((gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2]);
            f0 = f;
            if (nl > 0.0) { o_n[0] = (float)(gr[0] / nl); o_n[1] = (float)(gr[1] / nl); o_n[2] = (float)(gr[2] / nl); }
            if constexpr (ATTRIBUTES) {
                if (out.albedo) {
                    double w[8], a[8]; tri_weights(cc.f, w);
#pragma unroll
                    for (int k = 0; k < 8; ++k) a[k] = g.alb[cc.c[k]];
                    o_alb = (float)tri_sum(w, a);
                }
            }
            if (prm.project) {
                double x[3] = {p0[0], p0[1], p0[2]};
                int it = 0;
                for (;;) {
                    if (fabs(f) <= prm.tol) {                                // converged: tested before each step
                        const double dx = x[0] - p0[0], dy = x[1] - p0[1], dz = x[2] - p0[2];
                        const double len = sqrt((dx * dx + dy * dy) + dz * dz);
                        dist = f0 > 0.0 ? len : (f0 < 0.0 ? -len : 0.0);
                        foot[0] = x[0]; foot[1] = x[1]; foot[2] = x[2];
                        status |= 2;
                        break;
                    }
                    if (it >= prm.max_steps || !(nl > 0.0)) break;
                    const double s = fmin(fmax(f * vs / nl, -vs), vs);       // Newton step along the gradient, at most one voxel long in the world
#pragma unroll
                    for (int a = 0; a < 3; ++a) x[a] = x[a] - s * (gr[a] / nl);
                    ++it;
                    if (!cell_of_point(g, cc, x)) break;
                    f = field(cc);
                    cell_gradient(cc, gr);
                    nl = sqrt((gr[0] * gr[0] + gr[1] * gr[1]) + gr[2] * gr[2]);
                }
                steps = it;
            }
        }
        if (out.sdf) out.sdf[i] = f0;
        if (out.normal) { out.normal[3 * i] = o_n[0]; out.normal[3 * i + 1] = o_n[1]; out.normal[3 * i + 2] = o_n[2]; }
        if (ATTRIBUTES && out.albedo) out.albedo[i] = o_alb;
        if (out.foot) { out.foot[3 * i] = foot[0]; out.foot[3 * i + 1] = foot[1]; out.foot[3 * i + 2] = foot[2]; }
        if (out.distance) out.distance[i] = dist;
        if (out.status) out.status[i] = status;
    }
    // (f0 and dist are 0 for the points that do not count)
    double sd[NSUM] = {fabs(f0), f0 * f0, fabs(dist), dist * dist}, mx[NMAX] = {fabs(f0), fabs(dist)};
    long long cn[NCNT] = {(long long)(status & 1), (long long)((status >> 1) & 1), steps};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < NSUM; ++k) sd[k] += __shfl_xor(sd[k], o);
#pragma unroll
        for (int k = 0; k < NMAX; ++k) mx[k] = fmax(mx[k], __shfl_xor(mx[k], o));
#pragma unroll
        for (int k = 0; k < NCNT; ++k) cn[k] += __shfl_xor(cn[k], o);
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NSUM; ++k) part_d[wave][k] = sd[k];
#pragma unroll
        for (int k = 0; k < NMAX; ++k) part_d[wave][NSUM + k] = mx[k];
#pragma unroll
        for (int k = 0; k < NCNT; ++k) part_c[wave][k] = cn[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double d[NSUM + NMAX]; long long c[NCNT];
#pragma unroll
        for (int k = 0; k < NSUM; ++k) d[k] = ((part_d[0][k] + part_d[1][k]) + part_d[2][k]) + part_d[3][k];
#pragma unroll
        for (int k = NSUM; k < NSUM + NMAX; ++k) d[k] = fmax(fmax(part_d[0][k], part_d[1][k]), fmax(part_d[2][k], part_d[3][k]));
#pragma unroll
        for (int k = 0; k < NCNT; ++k) c[k] = ((part_c[0][k] + part_c[1][k]) + part_c[2][k]) + part_c[3][k];
        rows[blockIdx.x] = QueryRow{d[0], d[1], d[4], d[2], d[3], d[5], c[0], c[1], c[2]};
    }
}

__device__ inline void row_add(QueryRow& a, const QueryRow& b) {
    a.sum_abs_sdf += b.sum_abs_sdf; a.sum_sq_sdf += b.sum_sq_sdf; a.max_abs_sdf = fmax(a.max_abs_sdf, b.max_abs_sdf);
    a.sum_abs_distance += b.sum_abs_distance; a.sum_sq_distance += b.sum_sq_distance; a.max_abs_distance = fmax(a.max_abs_distance, b.max_abs_distance);
    a.valid += b.valid; a.projected += b.projected; a.steps += b.steps;
}

__global__ void __launch_bounds__(QUERY_BLOCK) k_query_reduce(const QueryRow* __restrict__ rows, int n, QueryRow* __restrict__ total) {
    __shared__ QueryRow part[QUERY_BLOCK];
    QueryRow acc{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0};
    for (int r = threadIdx.x; r < n; r += QUERY_BLOCK) row_add(acc, rows[r]);
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        QueryRow t = part[0];
        for (int k = 1; k < QUERY_BLOCK; ++k) row_add(t, part[k]);
        *total = t;
    }
}

template <class G>
void launch(hipStream_t st, const G& g, const QueryParams& p, const double* points, const QueryOut& out, QueryRow* rows, QueryRow* total) {
    const int nr = query_rows(p.n);
    if (nr > 0) k_query<G><<<nr, QUERY_BLOCK, 0, st>>>(g, p, points, out, rows);
    k_query_reduce<<<1, QUERY_BLOCK, 0, st>>>(rows, nr, total);
}

}  // namespace

void launch_query(hipStream_t st, const RenderGrid& g, const QueryParams& p, const double* points, const QueryOut& out, QueryRow* rows, QueryRow* total) {
    launch(st, g, p, points, out, rows, total);
}
void launch_query(hipStream_t st, const FusionRenderGrid& g, const QueryParams& p, const double* points, const QueryOut& out, QueryRow* rows, QueryRow* total) {
    launch(st, g, p, points, out, rows, total);
}

}  // namespace i3d
