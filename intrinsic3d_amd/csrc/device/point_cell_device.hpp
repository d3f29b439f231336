// The cell of cell_device.hpp under a world point, and a residual's contribution to the normal equations of k_track_solve: one definition each.
#pragma once
#include "query_kernels.hpp"
#include "track_kernels.hpp"
#include "cell_device.hpp"

namespace i3d {

// the cell under the world point x: false without any lookup when a coordinate is not finite or |x / vs| >= 2^20 (the int conversion never sees such a value)
template <class G>
__device__ inline bool cell_of_point(const G& g, CellCache& cc, const double (&x)[3]) {
    double q[3]; int b[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        q[a] = x[a] / g.vs;
        if (!isfinite(x[a]) || !(fabs(q[a]) < QUERY_MAX_COORD)) return false;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) b[a] = (int)floor(q[a]);
    return cell_at(g, cc, q, b);
}

// one residual r with the Jacobian row J into a lane's sums: scale(J_a J_b) into the 21 upper-triangle entries row by row, scale(J_a r) into the six after them,
// r^2 into column sq and 1 into column sq + 1.  scale is the term's weight on a product: the identity, omega x, wg2 (omega x), wp2 x.  FIRST: the lane's sums are
// still zero and the row is stored instead of added (0.0 + x is not x for x = -0.0, so the compiler cannot drop the 29 additions itself)
template <bool FIRST = false, class Scale>
__device__ inline void add_normal_row(double (&s)[TRACK_COLS], const double (&J)[6], double r, int sq, Scale scale) {
    const auto put = [](double& acc, double x) { acc = FIRST ? x : acc + x; };
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) put(s[k++], scale(J[a] * J[b]));
#pragma unroll
    for (int a = 0; a < 6; ++a) put(s[21 + a], scale(J[a] * r));
    put(s[sq], r * r); put(s[sq + 1], 1.0);
}

}  // namespace i3d
