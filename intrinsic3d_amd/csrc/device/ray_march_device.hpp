// One ray on the stored field in fp64: the ray, its clip against the brick bitmap's box, the march of DESIGN.md 13.1 (items 3-5) and the attributes at a hit
// (items 5-6) or the stored colour there, one definition for every kernel that marches (k_render of render_kernels.hip: a ray per pixel
// of a camera; k_cast_rays of cast_rays_kernels.hip: the caller's own rays).  The files that include this are compiled with
// -ffp-contract=off: the numpy statements of the definitions (tests/render_twin.py, tests/cast_rays_twin.py, tests/color_twin.py) evaluate the same fp64
// expressions in the same order.
#pragma once
#include "render_kernels.hpp"
#include "cell_device.hpp"
#include <type_traits>

namespace i3d {

__device__ inline int brick_of(int k) { return k >> RENDER_BRICK_SHIFT; }      // floor(k / 8)

struct Ray { double eye[3], dir[3], inv_len; };

// the position under the ray at t in voxel units q = (eye + t d) / vs and its cell base = floor(q) (the cell itself: cell_device.hpp)
__device__ inline void ray_pos(const Ray& r, double vs, double t, double (&q)[3], int (&b)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { q[a] = (r.eye[a] + t * r.dir[a]) / vs; b[a] = (int)floor(q[a]); }
}

template <class G>
__device__ inline bool field_at(const G& g, const Ray& r, CellCache& cc, double t, double& f) {
    double q[3]; int b[3]; ray_pos(r, g.vs, t, q, b);
    if (!cell_at(g, cc, q, b)) return false;
    f = field(cc);
    return true;
}

// [t0, t1) on entry: the ray's own range; on exit: clipped to the bitmap's box [8 lo, 8 (lo + dim)) in voxel units (t1 = -1: the ray runs beside the box)
template <class G>
__device__ inline void ray_clip(const G& g, const Ray& r, double& t0, double& t1) {
    const double vs = g.vs;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double B0 = (double)(g.lo[a] * 8) * vs, B1 = (double)((g.lo[a] + g.dim[a]) * 8) * vs;
        if (r.dir[a] != 0.0) {
            const double ta = (B0 - r.eye[a]) / r.dir[a], tb = (B1 - r.eye[a]) / r.dir[a];
            t0 = fmax(t0, fmin(ta, tb)); t1 = fmin(t1, fmax(ta, tb));
        } else if (r.eye[a] < B0 || r.eye[a] >= B1) {
            t1 = -1.0;
        }
    }
}

// the march of DESIGN.md 13.1, steps 3-5, over [tmin, tmax) in units of r.dir; returns the hit and leaves the cell of the attributes in cc
template <class G>
__device__ inline bool march(const G& g, double tmin, double tmax, const Ray& r, CellCache& cc, double& t_hit, int& samples) {
    const double vs = g.vs, dl = vs * r.inv_len;          // one voxel of world length along the ray, in units of t (the renderer's: camera z)
    double t0 = tmin, t1 = tmax;
    ray_clip(g, r, t0, t1);
    bool pv = false; double pt = 0.0, pf = 0.0;
    double t = t0;
    while (t < t1 && samples < RENDER_MAX_SAMPLES) {
        ++samples;
        double q[3]; int b[3]; ray_pos(r, vs, t, q, b);
        const int kx = brick_of(b[0]) - g.lo[0], ky = brick_of(b[1]) - g.lo[1], kz = brick_of(b[2]) - g.lo[2];
        if (kx < 0 || ky < 0 || kz < 0 || kx >= g.dim[0] || ky >= g.dim[1] || kz >= g.dim[2]) { pv = false; t += 1e-4 * dl; continue; }
        const long long bi = ((long long)kz * g.dim[1] + ky) * g.dim[0] + kx;
        if (!((g.bits[bi >> 5] >> (unsigned)(bi & 31)) & 1u)) {          // empty brick: jump to its exit
            double te = t1;
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (r.dir[a] != 0.0) {
                    const int kb = brick_of(b[a]);
                    const double edge = (double)((r.dir[a] > 0.0 ? kb + 1 : kb) * 8) * vs;
                    te = fmin(te, (edge - r.eye[a]) / r.dir[a]);
                }
            pv = false; t = fmax(t, te) + 1e-4 * dl;
            continue;
        }
        if (!cell_at(g, cc, q, b)) { pv = false; t += 0.5 * dl; continue; }
        const double f = field(cc);
        if (f > 0.0) { pv = true; pt = t; pf = f; t += fmin(fmax(f, 0.25 * vs), vs) * r.inv_len; continue; }
        if (pv && pf > 0.0) {                                               // zero crossing from outside: two secant steps on [pt, t]
            double ta = pt, fa = pf, tb = t, fb = f;
            const double tc = ta + (tb - ta) * fa / (fa - fb);
            double fc;
            if (!field_at(g, r, cc, tc, fc)) { t_hit = tc; }
            else {
                if (fc > 0.0) { ta = tc; fa = fc; } else { tb = tc; fb = fc; }
                t_hit = ta + (tb - ta) * fa / (fa - fb);
            }
            double fh;
            if (!field_at(g, r, cc, t_hit, fh)) field_at(g, r, cc, t, fh);  // attributes from the hit sample's cell when t_hit's cell is not valid
            return true;
        }
        pv = true; pt = t; pf = f; t += 0.25 * dl;
    }
    return false;
}

// the attributes of DESIGN.md 13.1 items 5-6 at the cell the march left in cc: the unit gradient, and in the context's grid (the only one with albedo / SH)
// the trilinear albedo and the shading under the trilinear SH.  want_albedo: an albedo or an SH plane is asked for; need_sh: an SH plane is
struct HitAttr { float n[3]; float albedo, shading, intensity; };

template <class G>
__device__ inline void hit_attributes(const G& g, const CellCache& cc, bool want_albedo, bool need_sh, HitAttr& o) {
    constexpr bool ATTRIBUTES = std::is_same<G, RenderGrid>::value;
    double w[8]; tri_weights(cc.f, w);
    double gr[3]; cell_gradient(cc, gr);
    const double nx = gr[0], ny = gr[1], nz = gr[2];
    const double nl = sqrt((nx * nx + ny * ny) + nz * nz);
    double n[3] = {0.0, 0.0, 0.0};
    if (nl > 0.0) { n[0] = nx / nl; n[1] = ny / nl; n[2] = nz / nl; }
    double alb = 0.0;
    double shade = 0.0;
    if constexpr (ATTRIBUTES) {
        if (want_albedo) {
            double a[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] = g.alb[cc.c[i]];
            alb = tri_sum(w, a);
        }
        if (need_sh && nl > 0.0) {
            const double H[9] = {1.0, n[1], n[2], n[0], n[0] * n[1], n[1] * n[2], -n[0] * n[0] - n[1] * n[1] + 2.0 * n[2] * n[2], n[0] * n[2], n[0] * n[0] - n[1] * n[1]};
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                double s[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) s[i] = (double)g.sh[(size_t)j * g.N + cc.c[i]];
                shade = shade + tri_sum(w, s) * H[j];
            }
        }
    }
    o.n[0] = (float)n[0]; o.n[1] = (float)n[1]; o.n[2] = (float)n[2];
    o.albedo = (float)alb; o.shading = (float)shade; o.intensity = (float)(alb * shade);
}

// the stored colour of corner c of the cell the march left in cc: a voxel of the context's grid, a slot of the fusion table (x = R, y = G, z = B in both; a slot
// that received depth but never colour holds 0, 0, 0: black, the rule of DESIGN.md 22)
__device__ inline uchar4 corner_color(const RenderGrid& g, int c) { return g.color[c]; }
__device__ inline uchar4 corner_color(const FusionRenderGrid& g, int c) { return g.t.color[c]; }

// the colour at a hit: per channel the stored byte widened to fp64 and interpolated with the weights and the sum albedo gets above; R, G, B
// in units of the byte, unrounded
template <class G>
__device__ inline void hit_color(const G& g, const CellCache& cc, float (&rgb)[3]) {
    double w[8]; tri_weights(cc.f, w);
    uchar4 c8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) c8[i] = corner_color(g, cc.c[i]);
    double a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = (double)c8[i].x;
    rgb[0] = (float)tri_sum(w, a);
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = (double)c8[i].y;
    rgb[1] = (float)tri_sum(w, a);
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = (double)c8[i].z;
    rgb[2] = (float)tri_sum(w, a);
}

}  // namespace i3d
