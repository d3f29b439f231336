// The fp64 pinhole camera with Brown distortion of the renderer and the trackers (render_kernels.hip, track_kernels.hip, track_sdf_kernels.hip): the struct, its
// construction on the host, and the one statement of its forward model, the model's derivative and its inverse.  The model is that of the fp32 observation pass
// (observe_device.hpp), whose y line reads the distorted x.  Translation units that use the device functions are compiled with -ffp-contract=off, and the numpy
// twins under tests/ restate the expressions in this order.
#pragma once
#include "common.hpp"
#include <cmath>

namespace i3d {

struct PinholeCam {                               // built on the host: camera_of, camera_at_level
    double fx, fy, cx, cy, dist[5];               // dist: k1 k2 k3 p1 p2
    int dist_zero, w, h;                          // dist_zero: every |dist| <= 1e-5, the model is the plain pinhole
};

inline PinholeCam camera_of(const double* intr4, const double* dist5, int w, int h) {
    PinholeCam k;
    k.fx = intr4[0]; k.fy = intr4[1]; k.cx = intr4[2]; k.cy = intr4[3];
    bool dz = true;
    for (int i = 0; i < 5; ++i) { k.dist[i] = dist5[i]; if (std::fabs(dist5[i]) > 1e-5) dz = false; }
    k.dist_zero = dz ? 1 : 0; k.w = w; k.h = h;
    return k;
}

// the camera of pyramid level l, whose image is w x h: make_params (assemble.cpp), all four intrinsics x 2^-level
inline PinholeCam camera_at_level(PinholeCam k, int l, int w, int h) {
    const double scale = 1.0 / std::pow(2.0, l);
    k.fx *= scale; k.fy *= scale; k.cx *= scale; k.cy *= scale;
    k.w = w; k.h = h;
    return k;
}

// the forward model on normalised coordinates, in place
__device__ inline void distort(const PinholeCam& c, double& x, double& y) {
    if (c.dist_zero) return;
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double dc = 1.0 + c.dist[0] * r2 + c.dist[1] * r4 + c.dist[2] * r6;
    x = x * dc + 2.0 * c.dist[3] * x * y + c.dist[4] * (r2 + 2.0 * x * x);
    y = y * dc + 2.0 * c.dist[4] * x * y + c.dist[3] * (r2 + 2.0 * y * y);
}

// d(xd, yd) / d(x, y) of distort at (x, y); the y row goes through xd, as the model does
__device__ inline void distort_jacobian(const PinholeCam& c, double x, double y, double& xx, double& xy, double& yx, double& yy) {
    xx = 1.0; xy = 0.0; yx = 0.0; yy = 1.0;
    if (c.dist_zero) return;
    const double k1 = c.dist[0], k2 = c.dist[1], k3 = c.dist[2], p1 = c.dist[3], p2 = c.dist[4];
    const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
    const double dc = 1.0 + k1 * r2 + k2 * r4 + k3 * r6;
    const double dr = (k1 + 2.0 * k2 * r2) + 3.0 * k3 * r4;          // d dc / d r2
    const double xd = x * dc + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
    xx = ((dc + x * (dr * (2.0 * x))) + 2.0 * p1 * y) + 6.0 * p2 * x;
    xy = (x * (dr * (2.0 * y)) + 2.0 * p1 * x) + 2.0 * p2 * y;
    yx = (y * (dr * (2.0 * x)) + 2.0 * p2 * (xx * y)) + 2.0 * p1 * x;
    yy = ((dc + y * (dr * (2.0 * y))) + 2.0 * p2 * (xy * y + xd)) + 6.0 * p1 * y;
}

// the ray of the integer pixel (u, v): the inverse of distort by 10 fixed-point iterations
__device__ inline void undistort(const PinholeCam& c, int u, int v, double& x, double& y) {
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
