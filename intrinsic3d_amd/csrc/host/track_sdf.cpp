// i3d_track_frame_sdf: registration of a depth frame on the stored field, no ray cast (track_sdf_kernels.hip; the definition is DESIGN.md section 19).
// track_sdf_run is the driver for every model (the context here, the fusion volume in fusion.cpp): validation, the camera, one grown-only scratch, one upload of
// the depth, the pivot, the whole budget launched back to back, the figures at the returned pose; two stream synchronisations.  The pose comes in and goes out
// world -> camera, as i3d_track_frame's; the loop runs on its inverse, the camera -> world pose of section 18.  Reads the grid and, with use_context_camera, the
// context's camera; writes only its scratch, nothing any other entry point reads.
#include "context.hpp"

using namespace i3d;

namespace {

constexpr int TRACK_SDF_MAX_EDGE = 1 << 15;
constexpr int TRACK_SDF_MAX_STRIDE = 16;
constexpr int TRACK_SDF_MAX_ITERATIONS = 200;

#define S_HIP(m, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (m).fail(I3D_ERR_HIP, std::string(#expr) + " -> " + hipGetErrorString(e_)); } while (0)

double rms_of(double sq, double n) { return n > 0.0 ? std::sqrt(sq / n) : 0.0; }

}  // namespace

namespace i3d {

int track_sdf_run(hipStream_t st, DevBuf<unsigned char>& scratch, const TrackSdfModel& m, const char* what, const i3d_track_sdf_desc* d, int32_t w, int32_t h,
                  const float* depth, double* pose6_io, i3d_track_sdf_stats* stats, const double* debug_pivot3, double* debug_sums29, int64_t* debug_valid,
                  int64_t* debug_usable) {
    const std::string fn(what);
    if (!d) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    if (!depth) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null depth");
    if (!pose6_io) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null pose");
    if (w <= 0 || h <= 0 || w > TRACK_SDF_MAX_EDGE || h > TRACK_SDF_MAX_EDGE) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": image size out of range");
    if (d->stride < 1 || d->stride > TRACK_SDF_MAX_STRIDE) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": stride must be 1.." + std::to_string(TRACK_SDF_MAX_STRIDE));
    if (d->iterations < 0 || d->iterations > TRACK_SDF_MAX_ITERATIONS)
        return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": iterations must be 0.." + std::to_string(TRACK_SDF_MAX_ITERATIONS));
    if (!std::isfinite(d->max_distance) || !(d->max_distance > 0.0)) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": max_distance must be finite and > 0");
    if (!std::isfinite(d->huber_delta)) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": huber_delta must be finite (<= 0: off)");
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(pose6_io[k])) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": the pose is not finite");
    const double* intr = d->intrinsics4; const double* dist = d->distortion5;
    if (int rc = m.ready(*d, intr, dist)) return rc;
    if (!d->use_context_camera && (!(intr[0] > 0.0) || !(intr[1] > 0.0))) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": focal lengths must be > 0");

    TrackSdfParams prm; std::memset(&prm, 0, sizeof(prm));
    TrackCam& k = prm.cam;
    k.fx = intr[0]; k.fy = intr[1]; k.cx = intr[2]; k.cy = intr[3];
    bool dz = true;
    for (int i = 0; i < 5; ++i) { k.dist[i] = dist[i]; if (std::fabs(dist[i]) > 1e-5) dz = false; }
    k.dist_zero = dz ? 1 : 0; k.w = w; k.h = h;
    const int ws = (w + d->stride - 1) / d->stride, hs_ = (h + d->stride - 1) / d->stride;
    const long long n = (long long)ws * hs_;
    prm.stride = d->stride; prm.ws = ws; prm.n = n;
    prm.min_depth = d->min_depth; prm.max_depth = d->max_depth;
    prm.max_distance = d->max_distance; prm.huber_delta = d->huber_delta;

    // the scratch: depth | slab | state; every piece 256-byte aligned
    const int P = register_per_lane(n, m.row_cap), rows = register_rows(n, P);
    prm.per_lane = P;
    const size_t px = (size_t)w * h;
    size_t total = 0;
    auto take = [&total](size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_depth = take(px * sizeof(float)), o_slab = take((size_t)rows * TRACK_COLS * sizeof(double)), o_state = take(sizeof(TrackState));
    S_HIP(m, scratch.alloc(total));
    const float* d_depth = (const float*)(scratch.p + o_depth);
    double* slab = (double*)(scratch.p + o_slab);
    TrackState* state = (TrackState*)(scratch.p + o_state);
    S_HIP(m, hipMemcpyAsync(scratch.p + o_depth, depth, px * sizeof(float), hipMemcpyHostToDevice, st));

    const Pose P0 = pose_from_vec6(pose6_io);               // camera -> world: x = R p + t
    const double* R0 = P0.R; const double* t0 = P0.t;
    TrackState hs; std::memset(&hs, 0, sizeof(hs));
    if (debug_pivot3) {
        for (int a = 0; a < 3; ++a) prm.c[a] = debug_pivot3[a];
    } else {                                                // the pivot: c = R0 mean(p) + t0 over the usable samples that count, fixed for the call
        launch_track_sdf_mean(st, prm, d_depth, R0, t0, m.voxel_size, slab);
        launch_track_solve(st, state, slab, rows, 1, 28, 0.0, 0.0);
        S_HIP(m, hipGetLastError());
        S_HIP(m, hipMemcpyAsync(&hs, state, sizeof(hs), hipMemcpyDeviceToHost, st));
        S_HIP(m, hipStreamSynchronize(st));
        double mean[3] = {0.0, 0.0, 0.0};
        if (hs.sums[3] > 0.0) for (int a = 0; a < 3; ++a) mean[a] = hs.sums[a] / hs.sums[3];
        for (int a = 0; a < 3; ++a) prm.c[a] = ((R0[3 * a] * mean[0] + R0[3 * a + 1] * mean[1]) + R0[3 * a + 2] * mean[2]) + t0[a];
    }
    std::memset(&hs, 0, sizeof(hs));
    for (int i = 0; i < 9; ++i) hs.R[i] = R0[i];
    for (int a = 0; a < 3; ++a) hs.t[a] = t0[a] - prm.c[a];
    hs.status = 1; hs.first = 1;
    S_HIP(m, hipMemcpyAsync(state, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
    const int budget = debug_pivot3 ? 0 : d->iterations;
    for (int it = 0; it < budget; ++it) {                   // back to back; once done is set the remaining launches return at once
        m.launch(prm, d_depth, state, 1, slab);
        launch_track_solve(st, state, slab, rows, 0, 28, d->stop_rotation, d->stop_translation);
    }
    m.launch(prm, d_depth, state, 0, slab);                 // the figures at the returned pose: totals only
    launch_track_solve(st, state, slab, rows, 1, 28, 0.0, 0.0);
    S_HIP(m, hipGetLastError());
    S_HIP(m, hipMemcpyAsync(&hs, state, sizeof(hs), hipMemcpyDeviceToHost, st));
    S_HIP(m, hipStreamSynchronize(st));
    if (debug_pivot3) {
        if (debug_sums29) for (int c = 0; c < TRACK_SUMS; ++c) debug_sums29[c] = hs.sums[c];
        if (debug_valid) *debug_valid = (int64_t)hs.sums[TRACK_SUMS];
        if (debug_usable) *debug_usable = (int64_t)hs.sums[TRACK_SDF_COL_USABLE];
        return I3D_OK;
    }
    i3d_track_sdf_stats out; std::memset(&out, 0, sizeof(out));
    out.valid_pixels = (int64_t)hs.sums[TRACK_SDF_COL_USABLE]; out.valid = (int64_t)hs.sums[TRACK_SUMS]; out.inliers = (int64_t)hs.sums[28];
    out.rms_final = rms_of(hs.sums[27], hs.sums[28]);
    out.rms_initial = budget > 0 ? hs.rms_first : out.rms_final;
    out.iterations = hs.iters;
    out.min_pivot_ratio = hs.min_pivot_ratio;
    out.status = budget > 0 ? hs.status : (out.inliers < TRACK_MIN_INLIERS ? 2 : 1);
    if (hs.iters > 0) {                                     // no step applied: the pose is left as it came in, bit for bit
        Pose Pn;
        for (int i = 0; i < 9; ++i) Pn.R[i] = hs.R[i];
        for (int a = 0; a < 3; ++a) Pn.t[a] = hs.t[a] + prm.c[a];
        vec6_from_pose(Pn, pose6_io);
    }
    if (stats) *stats = out;
    return I3D_OK;
}

}  // namespace i3d

namespace {

TrackSdfModel context_model(i3d_context* c, const i3d_track_sdf_desc* d, const std::string fn) {
    TrackSdfModel m;
    m.fail = [c](int code, const std::string& msg) { return ctx_fail(c, code, msg); };
    m.ready = [c, fn](const i3d_track_sdf_desc& dd, const double*& intr, const double*& dist) -> int {
        if (!c->have_grid) return ctx_fail(c, I3D_ERR_STATE, fn + ": no grid");
        if (dd.use_context_camera) {
            if (!c->have_camera) return ctx_fail(c, I3D_ERR_STATE, fn + ": use_context_camera without a camera (i3d_set_camera)");
            intr = c->intr; dist = c->dist;
        }
        CTX_HIP(c, hipSetDevice(c->device));
        return I3D_OK;
    };
    const bool refined = d && d->use_refined_sdf != 0;
    m.launch = [c, refined](const TrackSdfParams& p, const float* depth, const TrackState* state, int check_done, double* slab) {
        const RenderGrid g{HashTable{c->hkeys.p, c->hvals.p, c->hmask}, c->nbr.p, c->N, c->weight.p, refined ? c->x_sdf.p : c->sdf0.p, c->x_alb.p, c->sh.p,
                           (double)c->voxel_size, nullptr, {0, 0, 0}, {0, 0, 0}};
        launch_track_sdf(c->stream, g, p, depth, state, check_done, slab);
    };
    m.voxel_size = (double)c->voxel_size;
    m.row_cap = c->register_row_cap;
    return m;
}

}  // namespace

extern "C" void i3d_track_sdf_desc_default(i3d_track_sdf_desc* d) {
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    d->use_refined_sdf = 1; d->iterations = 30; d->stride = 1; d->max_distance = 0.05; d->stop_rotation = 1e-6; d->stop_translation = 1e-6;
}

extern "C" int i3d_track_frame_sdf(i3d_context* c, const i3d_track_sdf_desc* d, int32_t w, int32_t h, const float* depth, double* pose6_io,
                                   i3d_track_sdf_stats* stats) {
    const char* fn = "i3d_track_frame_sdf";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null context");
    return track_sdf_run(c->stream, c->track_sdf_scratch, context_model(c, d, fn), fn, d, w, h, depth, pose6_io, stats);
}

extern "C" int i3d_debug_track_sdf_sums(i3d_context* c, const i3d_track_sdf_desc* d, int32_t w, int32_t h, const float* depth, const double* pose6,
                                        const double* pivot3, double* sums29, int64_t* valid, int64_t* valid_pixels) {
    const char* fn = "i3d_debug_track_sdf_sums";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null context");
    if (!pose6 || !pivot3 || !sums29) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null argument");
    double pose[6];
    for (int k = 0; k < 6; ++k) pose[k] = pose6[k];
    return track_sdf_run(c->stream, c->track_sdf_scratch, context_model(c, d, fn), fn, d, w, h, depth, pose, nullptr, pivot3, sums29, valid, valid_pixels);
}
