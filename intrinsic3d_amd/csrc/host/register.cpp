// i3d_register_points: rigid alignment of a point set to the stored field by Gauss-Newton on f(R p + t) (register_kernels.hip; the definition is DESIGN.md
// section 18).  register_run is the driver for every model (model.hpp: the context here, the fusion volume in fusion.cpp): validation, the model's grown-only
// scratch, one upload of the points, then register_loop: the pivot, the whole budget launched back to back, the figures at the returned pose; two stream
// synchronisations.  register_loop serves the volume-to-volume registration as well (fusion_register_volume.cpp).  Reads the grid; writes only its scratch,
// nothing any other entry point reads.
#include "context.hpp"
#include "../device/frame_math.hpp"

using namespace i3d;

namespace {

constexpr int64_t REGISTER_MAX_POINTS = 1ll << 27;
constexpr int REGISTER_MAX_ITERATIONS = 200;

}  // namespace

namespace i3d {

void pivot_of(const double* sums, const double* R0, const double* t0, double* c) {
    double mean[3] = {0.0, 0.0, 0.0};
    if (sums[3] > 0.0) for (int a = 0; a < 3; ++a) mean[a] = sums[a] / sums[3];
    for (int a = 0; a < 3; ++a) c[a] = ((R0[3 * a] * mean[0] + R0[3 * a + 1] * mean[1]) + R0[3 * a + 2] * mean[2]) + t0[a];
}

void start_state(TrackState& hs, const double* R0, const double* t0, const double* c) {
    std::memset(&hs, 0, sizeof(hs));
    for (int i = 0; i < 9; ++i) hs.R[i] = R0[i];
    for (int a = 0; a < 3; ++a) hs.t[a] = t0[a] - c[a];
    hs.status = 1; hs.first = 1;
}

int register_loop(const Model& m, const RegisterLoop& lp, double* pose6_io, i3d_register_stats& out) {
    hipStream_t st = m.stream;
    const int rows = register_rows(lp.n, lp.per_lane);
    FrameConst fc; fm::frame_from_pose(pose6_io, fc);       // x = R p + t
    const double* R0 = fc.hot.R; const double* t0 = pose6_io + 3;
    TrackState hs; std::memset(&hs, 0, sizeof(hs));
    RegisterParams prm; prm.n = lp.n; prm.per_lane = lp.per_lane; prm.max_distance = lp.max_distance;
    if (lp.debug_pivot3) {
        for (int a = 0; a < 3; ++a) prm.c[a] = lp.debug_pivot3[a];
    } else {                                                // the pivot: c = R0 mean(p) + t0 over the points that count, fixed for the call
        lp.mean(R0, t0);
        launch_track_solve(st, lp.state, lp.slab, 1, rows, 1, 28, 0.0, 0.0);
        MODEL_HIP(m, hipGetLastError());
        MODEL_HIP(m, hipMemcpyAsync(&hs, lp.state, sizeof(hs), hipMemcpyDeviceToHost, st));
        MODEL_HIP(m, hipStreamSynchronize(st));
        pivot_of(hs.sums, R0, t0, prm.c);
    }
    start_state(hs, R0, t0, prm.c);
    MODEL_HIP(m, hipMemcpyAsync(lp.state, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
    const int budget = lp.debug_pivot3 ? 0 : lp.iterations;
    for (int it = 0; it < budget; ++it) {                   // back to back; once done is set the remaining launches return at once
        lp.pass(prm, 1);
        launch_track_solve(st, lp.state, lp.slab, 1, rows, 0, 28, lp.stop_rotation, lp.stop_translation);
    }
    lp.pass(prm, 0);                                        // the figures at the returned pose: totals only
    launch_track_solve(st, lp.state, lp.slab, 1, rows, 1, 28, 0.0, 0.0);
    MODEL_HIP(m, hipGetLastError());
    MODEL_HIP(m, hipMemcpyAsync(&hs, lp.state, sizeof(hs), hipMemcpyDeviceToHost, st));
    MODEL_HIP(m, hipStreamSynchronize(st));
    if (lp.debug_pivot3) {
        if (lp.debug_sums29) for (int k = 0; k < TRACK_SUMS; ++k) lp.debug_sums29[k] = hs.sums[k];
        if (lp.debug_valid) *lp.debug_valid = (int64_t)hs.sums[TRACK_SUMS];
        return I3D_OK;
    }
    out.valid = (int64_t)hs.sums[TRACK_SUMS]; out.inliers = (int64_t)hs.sums[28];
    out.rms_final = rms_of(hs.sums[27], hs.sums[28]);
    out.rms_initial = budget > 0 ? hs.rms_first : out.rms_final;
    out.iterations = hs.iters;
    out.min_pivot_ratio = hs.min_pivot_ratio;
    out.status = budget > 0 ? hs.status : (out.inliers < TRACK_MIN_INLIERS ? 2 : 1);
    if (hs.iters > 0) {                                     // no step applied: the pose is left as it came in, bit for bit
        rot_to_aa(hs.R, pose6_io);
        for (int a = 0; a < 3; ++a) pose6_io[3 + a] = hs.t[a] + prm.c[a];
    }
    return I3D_OK;
}

int register_run(const Model& m, const i3d_register_desc* d, int64_t n, const double* points, double* pose6_io, i3d_register_stats* stats, const double* debug_pivot3,
                 double* debug_sums29, int64_t* debug_valid) {
    const std::string& fn = m.fn;
    hipStream_t st = m.stream; DevBuf<unsigned char>& scratch = m.buf.register_scratch;
    if (!d) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    if (!pose6_io) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null pose");
    if (n < 0 || n > REGISTER_MAX_POINTS) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": n must be 0.." + std::to_string(REGISTER_MAX_POINTS) + " (2^27)");
    if (n > 0 && !points) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null points");
    if (d->iterations < 0 || d->iterations > REGISTER_MAX_ITERATIONS)
        return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": iterations must be 0.." + std::to_string(REGISTER_MAX_ITERATIONS));
    if (!std::isfinite(d->max_distance) || !(d->max_distance > 0.0)) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": max_distance must be finite and > 0");
    if (int rc = m.check_pose(pose6_io)) return rc;
    if (int rc = m.ready()) return rc;
    i3d_register_stats out; std::memset(&out, 0, sizeof(out));
    out.status = 2;
    if (debug_sums29) std::memset(debug_sums29, 0, TRACK_SUMS * sizeof(double));
    if (debug_valid) *debug_valid = 0;
    if (n == 0) { if (stats) *stats = out; return I3D_OK; }

    // the scratch: points | slab | state; every piece 256-byte aligned
    const int P = register_per_lane(n, m.row_cap), rows = register_rows(n, P);
    const size_t N = (size_t)n;
    size_t total = 0;
    auto take = [&total](size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_pts = take(24 * N), o_slab = take((size_t)rows * TRACK_COLS * sizeof(double)), o_state = take(sizeof(TrackState));
    MODEL_HIP(m, scratch.alloc(total));
    const double* d_pts = (const double*)(scratch.p + o_pts);
    double* slab = (double*)(scratch.p + o_slab);
    TrackState* state = (TrackState*)(scratch.p + o_state);
    MODEL_HIP(m, hipMemcpyAsync(scratch.p + o_pts, points, 24 * N, hipMemcpyHostToDevice, st));

    RegisterLoop lp;
    lp.slab = slab; lp.state = state; lp.n = (long long)n; lp.per_lane = P;
    lp.mean = [&](const double* R0, const double* t0) { launch_register_mean(st, (long long)n, P, d_pts, R0, t0, m.voxel_size, slab); };
    lp.pass = [&](const RegisterParams& prm, int check_done) { m.register_pass(prm, d_pts, state, check_done, slab); };
    lp.iterations = d->iterations; lp.stop_rotation = d->stop_rotation; lp.stop_translation = d->stop_translation; lp.max_distance = d->max_distance;
    lp.debug_pivot3 = debug_pivot3; lp.debug_sums29 = debug_sums29; lp.debug_valid = debug_valid;
    if (int rc = register_loop(m, lp, pose6_io, out)) return rc;
    if (stats && !debug_pivot3) *stats = out;
    return I3D_OK;
}

}  // namespace i3d

extern "C" void i3d_register_desc_default(i3d_register_desc* d) {
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    d->use_refined_sdf = 1; d->iterations = 30; d->max_distance = 0.05; d->stop_rotation = 1e-6; d->stop_translation = 1e-6;
}

extern "C" int i3d_register_points(i3d_context* c, const i3d_register_desc* d, int64_t n, const double* points, double* pose6_io, i3d_register_stats* stats) {
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_register_points: null context");
    return register_run(ContextModel(c, "i3d_register_points", d && d->use_refined_sdf != 0), d, n, points, pose6_io, stats);
}

extern "C" int i3d_debug_register_sums(i3d_context* c, const i3d_register_desc* d, int64_t n, const double* points, const double* pose6, const double* pivot3,
                                       double* sums29, int64_t* valid) {
    const char* fn = "i3d_debug_register_sums";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null context");
    if (!pose6 || !pivot3 || !sums29) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null argument");
    double pose[6];
    for (int k = 0; k < 6; ++k) pose[k] = pose6[k];
    return register_run(ContextModel(c, fn, d && d->use_refined_sdf != 0), d, n, points, pose, nullptr, pivot3, sums29, valid);
}

extern "C" int i3d_debug_register_row_cap(i3d_context* c, int32_t rows) {
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_debug_register_row_cap: null context");
    if (rows < 0 || rows > REGISTER_MAX_ROWS) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_debug_register_row_cap: rows must be 0..8192 (0: the default)");
    c->register_row_cap = rows == 0 ? REGISTER_MAX_ROWS : rows;
    return I3D_OK;
}
