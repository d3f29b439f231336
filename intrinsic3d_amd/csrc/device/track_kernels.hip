// Projective point-to-plane ICP of a depth frame against the resident model (i3d_track_frame; the definition is DESIGN.md section 14).
//   k_track_points  one lane per pixel of a frame pyramid level: back-projection through the renderer's undistortion, normal from the right / lower neighbours
//   k_track_assoc<PHOTO>  one lane per frame pixel: association with the model planes of the level's ray cast, residual, Jacobian, the 29 fp64 sums + the
//                   valid-pixel count; summed over the wave by a reduce-scatter butterfly of shuffles, over the workgroup through LDS; one slab row per workgroup.
//                   PHOTO (i3d_track_frame_rgbd): the geometric contribution scaled by wg2, then the photometric residual against the
//                   cast's intensity plane, scaled by wp2
//   k_track_solve   one workgroup per loop (one, or the frames of a batch): the slab summed in a fixed order, 6x6 Cholesky in fp64, the pose composed in device memory, the done flag set
// No float atomics: every sum has a fixed order, so results are bit-reproducible run to run.  Compiled with -ffp-contract=off: the numpy statement of the
// definition (tests/track_twin.py) evaluates the same fp64 expressions in the same order.
#include "track_kernels.hpp"
#include "point_cell_device.hpp"    // add_normal_row
#include "slab_device.hpp"          // slab_row

namespace i3d {
namespace {

__device__ inline bool frame_point(const PinholeCam& c, const float* __restrict__ depth, float min_depth, float max_depth, int u, int v, double (&p)[3]) {
    const float z = depth[(size_t)v * c.w + u];
    if (!(z > 0.0f) || (min_depth > 0.0f && z < min_depth) || (max_depth > 0.0f && z > max_depth)) return false;
    double x, y; undistort(c, u, v, x, y);
    const double zd = (double)z;
    p[0] = x * zd; p[1] = y * zd; p[2] = zd;
    return true;
}

__global__ void __launch_bounds__(256) k_track_points(PinholeCam c, const float* __restrict__ depth, float min_depth, float max_depth, float* __restrict__ vtx,
                                                      float* __restrict__ nrm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.w * c.h) return;
    const int u = i % c.w, v = i / c.w;
    double p[3], pr[3], pd[3], n[3] = {0.0, 0.0, 0.0};
    bool ok = u + 1 < c.w && v + 1 < c.h && frame_point(c, depth, min_depth, max_depth, u, v, p) && frame_point(c, depth, min_depth, max_depth, u + 1, v, pr) &&
              frame_point(c, depth, min_depth, max_depth, u, v + 1, pd);
    if (ok) {
        const double a0 = pr[0] - p[0], a1 = pr[1] - p[1], a2 = pr[2] - p[2];          // to the right neighbour
        const double b0 = pd[0] - p[0], b1 = pd[1] - p[1], b2 = pd[2] - p[2];          // to the lower neighbour
        const double nx = b1 * a2 - b2 * a1, ny = b2 * a0 - b0 * a2, nz = b0 * a1 - b1 * a0;   // (lower x right): towards the camera
        const double nl = sqrt((nx * nx + ny * ny) + nz * nz);
        if (nl > 0.0) { n[0] = nx / nl; n[1] = ny / nl; n[2] = nz / nl; } else ok = false;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { vtx[3 * (size_t)i + a] = ok ? (float)p[a] : 0.0f; nrm[3 * (size_t)i + a] = ok ? (float)n[a] : 0.0f; }
}

// the association of DESIGN.md 14.1 item 4 for one valid frame point
struct Assoc {
    double p[3], q[3];                                              // the frame point in the world / in the camera of the ray cast
    double ud, vd;                                                  // its projection + 0.5
    double nm[3], dx, dy, dz;                                       // model normal, p - m
    float md; size_t mp;                                            // model depth and index of the associated model pixel
};

__device__ inline bool associate(const PinholeCam& c, const TrackRef& ref, const double (&Rc)[9], const double (&tc)[3], const float* __restrict__ vtx,
                                 const float* __restrict__ nrm, const float* __restrict__ mdepth, const float* __restrict__ mnormal, double max_d2, double min_dot,
                                 size_t i, double vz, Assoc& a) {
    const double vx = vtx[3 * i], vy = vtx[3 * i + 1];
    const double nvx = nrm[3 * i], nvy = nrm[3 * i + 1], nvz = nrm[3 * i + 2];
    double (&p)[3] = a.p; double (&q)[3] = a.q;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = ((Rc[3 * k] * vx + Rc[3 * k + 1] * vy) + Rc[3 * k + 2] * vz) + tc[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = ((ref.R[3 * k] * p[0] + ref.R[3 * k + 1] * p[1]) + ref.R[3 * k + 2] * p[2]) + ref.t[k];
    bool in = q[2] > 0.0;
    int ui = 0, vi = 0;
    if (in) {
        double x = q[0] / q[2], y = q[1] / q[2];
        distort(c, x, y);
        const double ud = (c.fx * x + c.cx) + 0.5, vd = (c.fy * y + c.cy) + 0.5;
        in = ud > -1.0 && ud < (double)c.w && vd > -1.0 && vd < (double)c.h;     // (int)(u + 0.5) in [0, w) without an out-of-range conversion
        if (in) { ui = (int)ud; vi = (int)vd; }
        a.ud = ud; a.vd = vd;
    }
    const size_t mp = (size_t)vi * c.w + ui;
    const float md = in ? mdepth[mp] : 0.0f;
    if (!(md > 0.0f)) return false;
    const double nm0 = mnormal[3 * mp], nm1 = mnormal[3 * mp + 1], nm2 = mnormal[3 * mp + 2];
    double x, y; undistort(c, ui, vi, x, y);
    double d[3], m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { d[k] = (ref.R[k] * x + ref.R[3 + k] * y) + ref.R[6 + k]; m[k] = ref.eye[k] + (double)md * d[k]; }
    const double dx = p[0] - m[0], dy = p[1] - m[1], dz = p[2] - m[2];
    const double d2 = (dx * dx + dy * dy) + dz * dz;
    const double nw0 = (Rc[0] * nvx + Rc[1] * nvy) + Rc[2] * nvz, nw1 = (Rc[3] * nvx + Rc[4] * nvy) + Rc[5] * nvz, nw2 = (Rc[6] * nvx + Rc[7] * nvy) + Rc[8] * nvz;
    const double dot = (nm0 * nw0 + nm1 * nw1) + nm2 * nw2;
    a.nm[0] = nm0; a.nm[1] = nm1; a.nm[2] = nm2; a.dx = dx; a.dy = dy; a.dz = dz; a.md = md; a.mp = mp;
    return (nm0 != 0.0 || nm1 != 0.0 || nm2 != 0.0) && d2 <= max_d2 && dot >= min_dot;
}

// the photometric term of DESIGN.md 16 for the associated frame pixel i: the frame's luminance against the bilinear interpolant of the model's intensity plane
// at the projection of the frame point.  A lane without a photometric sample adds nothing
__device__ inline void add_photo_row(const PinholeCam& c, const TrackRef& ref, const TrackPhoto& ph, const float* __restrict__ mdepth, const Assoc& a, int i,
                                     double (&s)[TRACK_COLS]) {
    // continuous model-image coordinates, the four pixels of the bilinear cell; ud in (-1, w) keeps the conversions in range
    // a coordinate within 1e-9 pixel of a pixel centre is that centre (fraction 0 of the cell to its right / below): at a pass's first association every point
    // projects onto its own pixel to rounding, and the side of the cell corner must not fall to the last bit
    double us = a.ud - 0.5, vs = a.vd - 0.5;
    const double ur = rint(us), vr = rint(vs);
    if (fabs(us - ur) < 1e-9) us = ur;
    if (fabs(vs - vr) < 1e-9) vs = vr;
    const double xf = floor(us), yf = floor(vs);
    const int x0 = (int)xf, y0 = (int)yf;
    if (!(ph.mintensity && x0 >= 0 && y0 >= 0 && x0 + 1 < c.w && y0 + 1 < c.h)) return;
    const size_t o = (size_t)y0 * c.w + x0;
    const float d00 = mdepth[o], d10 = mdepth[o + 1], d01 = mdepth[o + c.w], d11 = mdepth[o + c.w + 1];
    const double md = (double)a.md;
    if (!(d00 > 0.0f && d10 > 0.0f && d01 > 0.0f && d11 > 0.0f && fabs((double)d00 - md) <= ph.max_distance && fabs((double)d10 - md) <= ph.max_distance &&
          fabs((double)d01 - md) <= ph.max_distance && fabs((double)d11 - md) <= ph.max_distance))
        return;
    const double I00 = ph.mintensity[o], I10 = ph.mintensity[o + 1], I01 = ph.mintensity[o + c.w], I11 = ph.mintensity[o + c.w + 1];
    const double fx = us - xf, fy = vs - yf, gx = 1.0 - fx, gy = 1.0 - fy;
    const double Im = gy * (gx * I00 + fx * I10) + fy * (gx * I01 + fx * I11);
    const double gu = gy * (I10 - I00) + fy * (I11 - I01), gv = gx * (I01 - I00) + fx * (I11 - I10);
    const double rp = Im - (double)ph.lum[i];
    if (ph.max_residual > 0.0 && !(fabs(rp) <= ph.max_residual)) return;
    const double* p = a.p; const double* q = a.q;
    const double x = q[0] / q[2], y = q[1] / q[2];
    double xx, xy, yx, yy; distort_jacobian(c, x, y, xx, xy, yx, yy);
    const double hx = gu * (c.fx * xx) + gv * (c.fy * yx), hy = gu * (c.fx * xy) + gv * (c.fy * yy);      // g^T d(u, v) / d(x, y)
    const double gq0 = hx / q[2], gq1 = hy / q[2], gq2 = -(hx * x + hy * y) / q[2];
    double av[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) av[k] = (ref.R[k] * gq0 + ref.R[3 + k] * gq1) + ref.R[6 + k] * gq2;       // a = R_ref^T J_pi^T g
    const double J[6] = {p[1] * av[2] - p[2] * av[1], p[2] * av[0] - p[0] * av[2], p[0] * av[1] - p[1] * av[0], av[0], av[1], av[2]};
    const double wp2 = ph.wp2;
    add_normal_row(s, J, rp, TRACK_COL_PHOTO_SQ, [wp2](double x_) { return wp2 * x_; });
}

// ph is read with PHOTO only.  With wg2 = 1 and no intensity plane the sums of PHOTO are those without it bit for bit (1.0 * x is exact)
template <bool PHOTO>
__global__ void __launch_bounds__(TRACK_BLOCK) k_track_assoc(PinholeCam c, TrackRef ref, const float* __restrict__ vtx, const float* __restrict__ nrm,
                                                             const float* __restrict__ mdepth, const float* __restrict__ mnormal, TrackPhoto ph, double max_d2,
                                                             double min_dot, const TrackState* __restrict__ st, int check_done, double* __restrict__ slab) {
    __shared__ double part[TRACK_BLOCK / 64][TRACK_COLS];
    if (check_done && st->done) return;
    double Rc[9], tc[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) Rc[i] = st->R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) tc[i] = st->t[i];
    const int i = blockIdx.x * TRACK_BLOCK + threadIdx.x;
    double s[TRACK_COLS];
#pragma unroll
    for (int k = 0; k < TRACK_COLS; ++k) s[k] = 0.0;
    if (i < c.w * c.h) {                                 // tail lanes fall through to the shuffles with zeros
        const double vz = vtx[3 * (size_t)i + 2];
        if (vz > 0.0) {
            s[29] = 1.0;
            Assoc a;
            if (associate(c, ref, Rc, tc, vtx, nrm, mdepth, mnormal, max_d2, min_dot, (size_t)i, vz, a)) {
                const double* p = a.p;
                const double nm0 = a.nm[0], nm1 = a.nm[1], nm2 = a.nm[2];
                const double r = (nm0 * a.dx + nm1 * a.dy) + nm2 * a.dz;
                const double J[6] = {p[1] * nm2 - p[2] * nm1, p[2] * nm0 - p[0] * nm2, p[0] * nm1 - p[1] * nm0, nm0, nm1, nm2};
                if constexpr (PHOTO) {
                    const double wg2 = ph.wg2;
                    add_normal_row<true>(s, J, r, 27, [wg2](double x) { return wg2 * x; });
                    add_photo_row(c, ref, ph, mdepth, a, i, s);
                } else {
                    add_normal_row<true>(s, J, r, 27, [](double x) { return x; });
                }
            }
        }
    }
    slab_row(s, part, slab);
}

constexpr int SOLVE_PARTS = 256 / TRACK_COLS;       // 8 strided partial sums per column

// workgroup f owns state f and the rows of slab f
__global__ void __launch_bounds__(256) k_track_solve(TrackState* __restrict__ st, const double* __restrict__ slab, int rows, int mode, int count_col,
                                                     double stop_rot, double stop_trans) {
    __shared__ double part[SOLVE_PARTS][TRACK_COLS];
    st += blockIdx.x;
    slab += (size_t)blockIdx.x * rows * TRACK_COLS;
    if (mode == 0 && st->done) return;
    const int col = threadIdx.x & (TRACK_COLS - 1), pi = threadIdx.x / TRACK_COLS;
    double acc = 0.0;
    for (int r = pi; r < rows; r += SOLVE_PARTS) acc += slab[(size_t)r * TRACK_COLS + col];
    part[pi][col] = acc;
    __syncthreads();
    if (threadIdx.x < TRACK_COLS) {
        double t = part[0][col];
#pragma unroll
        for (int k = 1; k < SOLVE_PARTS; ++k) t += part[k][col];
        st->sums[col] = t;
        part[0][col] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0 || mode != 0) return;
    double tot[TRACK_COLS];
#pragma unroll
    for (int k = 0; k < TRACK_COLS; ++k) tot[k] = part[0][k];
    const double cnt = tot[28], pcnt = tot[TRACK_COL_PHOTO_N];
    if (st->first) {
        st->rms_first = cnt > 0.0 ? sqrt(tot[27] / cnt) : 0.0;
        st->rms_first_photo = pcnt > 0.0 ? sqrt(tot[TRACK_COL_PHOTO_SQ] / pcnt) : 0.0;
        st->first = 0;
    }
    if ((count_col == TRACK_COL_PHOTO_N ? pcnt : cnt) < (double)TRACK_MIN_INLIERS) { st->status = 2; st->done = 1; return; }
    double A[6][6], L[6][6], b[6], piv[6];
    {
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c) { A[a][c] = tot[k]; A[c][a] = tot[k]; ++k; }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) b[a] = tot[21 + a];
    double trace = A[0][0];
#pragma unroll
    for (int a = 1; a < 6; ++a) trace = trace + A[a][a];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
        piv[j] = d;
        if (!(d > 1e-12 * trace)) {
            // degenerate: the factorisation stops at the first failing pivot; the ratio is that pivot, not below 0, over the largest pivot up to this column
            double pm = piv[0];
#pragma unroll
            for (int k = 1; k <= j; ++k) pm = fmax(pm, piv[k]);
            st->min_pivot_ratio = pm > 0.0 ? fmax(d, 0.0) / pm : 0.0;
            st->status = 3; st->done = 1;
            return;
        }
        L[j][j] = sqrt(fmax(d, 0.0));
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    double pmin = piv[0], pmax = piv[0];
#pragma unroll
    for (int j = 1; j < 6; ++j) { pmin = fmin(pmin, piv[j]); pmax = fmax(pmax, piv[j]); }
    st->min_pivot_ratio = pmax > 0.0 ? pmin / pmax : 0.0;
    double y[6], x[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double v = -b[i];
#pragma unroll
        for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * x[k];
        x[i] = v / L[i][i];
    }
    // T_cw <- exp(delta) T_cw with exp(omega, upsilon): p -> R(omega) p + upsilon, R(omega) by Rodrigues
    const double th2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2], th = sqrt(th2);
    const double ul = sqrt((x[3] * x[3] + x[4] * x[4]) + x[5] * x[5]);
    double Rd[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (th2 > 0.0) {
        const double k0 = x[0] / th, k1 = x[1] / th, k2 = x[2] / th, co = cos(th), si = sin(th), v = 1.0 - co;
        Rd[0] = co + k0 * k0 * v; Rd[1] = k0 * k1 * v - k2 * si; Rd[2] = k0 * k2 * v + k1 * si;
        Rd[3] = k1 * k0 * v + k2 * si; Rd[4] = co + k1 * k1 * v; Rd[5] = k1 * k2 * v - k0 * si;
        Rd[6] = k2 * k0 * v - k1 * si; Rd[7] = k2 * k1 * v + k0 * si; Rd[8] = co + k2 * k2 * v;
    }
    double Rn[9], tn[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Rn[3 * a + c] = (Rd[3 * a] * st->R[c] + Rd[3 * a + 1] * st->R[3 + c]) + Rd[3 * a + 2] * st->R[6 + c];
        tn[a] = ((Rd[3 * a] * st->t[0] + Rd[3 * a + 1] * st->t[1]) + Rd[3 * a + 2] * st->t[2]) + x[3 + a];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) st->R[k] = Rn[k];
#pragma unroll
    for (int a = 0; a < 3; ++a) st->t[a] = tn[a];
    st->iters = st->iters + 1;
    if (th < stop_rot && ul < stop_trans) { st->status = 0; st->done = 1; } else st->status = 1;
}

}  // namespace

void launch_track_points(hipStream_t st, const PinholeCam& cam, const float* depth, float min_depth, float max_depth, float* vtx, float* nrm) {
    const int n = cam.w * cam.h;
    if (n > 0) k_track_points<<<(n + 255) / 256, 256, 0, st>>>(cam, depth, min_depth, max_depth, vtx, nrm);
}
int track_assoc_rows(int w, int h) { return (w * h + TRACK_BLOCK - 1) / TRACK_BLOCK; }
void launch_track_assoc(hipStream_t st, const PinholeCam& cam, const TrackRef& ref, const float* vtx, const float* nrm, const float* mdepth, const float* mnormal,
                        const TrackPhoto* photo, double max_distance, double min_normal_dot, const TrackState* state, int check_done, double* slab) {
    const int rows = track_assoc_rows(cam.w, cam.h);
    const double max_d2 = max_distance * max_distance;
    if (rows <= 0) return;
    if (photo) k_track_assoc<true><<<rows, TRACK_BLOCK, 0, st>>>(cam, ref, vtx, nrm, mdepth, mnormal, *photo, max_d2, min_normal_dot, state, check_done, slab);
    else k_track_assoc<false><<<rows, TRACK_BLOCK, 0, st>>>(cam, ref, vtx, nrm, mdepth, mnormal, TrackPhoto{}, max_d2, min_normal_dot, state, check_done, slab);
}
void launch_track_solve(hipStream_t st, TrackState* states, const double* slab, int frames, int rows, int mode, int count_col, double stop_rotation,
                        double stop_translation) {
    if (frames > 0) k_track_solve<<<frames, 256, 0, st>>>(states, slab, rows, mode, count_col, stop_rotation, stop_translation);
}

}  // namespace i3d
