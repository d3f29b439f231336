// The cell of cell_device.hpp under a world point: one definition for the kernels that sample the field at points (query_kernels.hip, register_kernels.hip).
#pragma once
#include "query_kernels.hpp"
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

}  // namespace i3d
