// The undistorted ray of an integer pixel of a TrackCam: one definition for the kernels that back-project frame pixels (track_kernels.hip,
// track_sdf_kernels.hip).
#pragma once
#include "track_kernels.hpp"

namespace i3d {

// the ray of the integer pixel (u, v): undistortion = 10 fixed-point iterations of the forward model of observe_device.hpp, as k_render (render_kernels.hip)
__device__ inline void undistort(const TrackCam& c, int u, int v, double& x, double& y) {
    const double xd = ((double)u - c.cx) / c.fx, yd = ((double)v - c.cy) / c.fy;
    x = xd; y = yd;
    if (!c.dist_zero) {
        const double k1 = c.dist[0], k2 = c.dist[1], k3 = c.dist[2], p1 = c.dist[3], p2 = c.dist[4];
        for (int it = 0; it < 10; ++it) {
            const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
            const double dc = 1.0 + k1 * r2 + k2 * r4 + k3 * r6;
            const double xn = (xd - (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) / dc;
            const double yn = (yd - (2.0 * p2 * xd * y + p1 * (r2 + 2.0 * y * y))) / dc;
            x = xn; y = yn;
        }
    }
}

}  // namespace i3d
