// The tracking driver — validation, the camera of each pyramid level, grown-only device buffers and the coarse-to-fine loop of levels and passes (track_kernels.hip;
// the definition is DESIGN.md section 14; the photometric term of i3d_track_frame_rgbd is section 16) — and its context entry points i3d_track_frame /
// i3d_track_frame_rgbd / i3d_debug_track_sums / i3d_debug_track_rgbd_sums.  The driver asks a Model (model.hpp) for its checks, its camera and its ray cast (the
// context's grid here, the fusion volume in fusion.cpp).  Reads the model and, with use_context_camera, the context's camera; writes only the model's TrackBuffers
// (and its cached brick bitmap), nothing the optimiser or the fusion reads.
#include "context.hpp"
#include "../device/frame_math.hpp"
#include "../device/level_kernels.hpp"
#include <limits>

using namespace i3d;

namespace i3d {

// rotation (row-major) -> angle-axis, stable at small angles and near pi
void rot_to_aa(const double R[9], double aa[3]) {
    const double c = 0.5 * ((R[0] + R[4] + R[8]) - 1.0);
    const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double s = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double th = std::atan2(s, c);
    if (s > 1e-7 || c > 0.0) {
        const double f = s > 0.0 ? th / s : 1.0;
        for (int a = 0; a < 3; ++a) aa[a] = v[a] * f;
        return;
    }
    int i = 0; if (R[4] > R[0]) i = 1; if (R[8] > R[4 * i]) i = 2;                 // near pi: the axis from the largest diagonal entry
    double k[3];
    k[i] = std::sqrt(std::fmax(0.0, (R[4 * i] - c) / (1.0 - c)));
    for (int j = 0; j < 3; ++j) if (j != i) k[j] = (R[3 * i + j] + R[3 * j + i]) / (2.0 * k[i] * (1.0 - c));
    if (k[0] * v[0] + k[1] * v[1] + k[2] * v[2] < 0.0) for (int a = 0; a < 3; ++a) k[a] = -k[a];
    for (int a = 0; a < 3; ++a) aa[a] = k[a] * th;
}

Pose pose_from_vec6(const double* p6) {          // world -> camera angle-axis | t (the rotation of i3d_set_camera / the renderer) -> camera -> world
    FrameConst fc; fm::frame_from_pose(p6, fc);
    Pose P;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) P.R[3 * a + b] = fc.hot.R[3 * b + a];
    for (int a = 0; a < 3; ++a) P.t[a] = -((fc.hot.R[a] * fc.hot.t[0] + fc.hot.R[3 + a] * fc.hot.t[1]) + fc.hot.R[6 + a] * fc.hot.t[2]);
    return P;
}

void vec6_from_pose(const Pose& P, double* p6) {
    double R[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) R[3 * a + b] = P.R[3 * b + a];
    rot_to_aa(R, p6);
    for (int a = 0; a < 3; ++a) p6[3 + a] = -((R[3 * a] * P.t[0] + R[3 * a + 1] * P.t[1]) + R[3 * a + 2] * P.t[2]);
}

}  // namespace i3d

namespace {

constexpr int TRACK_MAX_LEVELS = 4;
constexpr int TRACK_MAX_ITERATIONS = 100;
constexpr int TRACK_MAX_EDGE = 1 << 15;
constexpr int TRACK_MIN_LEVEL_EDGE = 4;          // the coarsest level used must keep at least this many pixels per edge

TrackRef ref_from_pose(const Pose& P) {
    TrackRef r;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) r.R[3 * a + b] = P.R[3 * b + a];
    for (int a = 0; a < 3; ++a) { r.eye[a] = P.t[a]; r.t[a] = -((r.R[3 * a] * P.t[0] + r.R[3 * a + 1] * P.t[1]) + r.R[3 * a + 2] * P.t[2]); }
    return r;
}

// the per-call set-up shared by every entry point: validation, the level-0 camera, the frame depth pyramid on the device, the model's caches
struct Setup {
    PinholeCam cam0; int levels; size_t pyr_off[TRACK_MAX_LEVELS]; int lw[TRACK_MAX_LEVELS], lh[TRACK_MAX_LEVELS];
    const TrackRgbd* rgbd;                           // null: depth only
    bool photo() const { return rgbd && rgbd->photo_weight > 0.0; }
    int count_col() const { return rgbd && !(rgbd->geometric_weight > 0.0) ? TRACK_COL_PHOTO_N : 28; }       // what status 2 counts
};

int setup(const Model& m, const i3d_track_desc* d, int w, int h, const float* depth, int levels, const TrackRgbd* rgbd, Setup& s) {
    const std::string& fn = m.fn;
    hipStream_t st = m.stream; TrackBuffers& b = m.buf.track;
    s.rgbd = rgbd;
    if (!d) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    if (!depth) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null depth");
    if (rgbd) {
        if (!rgbd->luminance) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null luminance");
        if (int rc = m.check_weights(rgbd->geometric_weight, rgbd->photo_weight)) return rc;
    }
    if (d->levels < 1 || d->levels > TRACK_MAX_LEVELS) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": levels must be 1.." + std::to_string(TRACK_MAX_LEVELS));
    for (int l = 0; l < d->levels; ++l)
        if (d->iterations[l] < 0 || d->iterations[l] > TRACK_MAX_ITERATIONS)
            return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": iterations must be 0.." + std::to_string(TRACK_MAX_ITERATIONS));
    if (w <= 0 || h <= 0 || w > TRACK_MAX_EDGE || h > TRACK_MAX_EDGE) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": image size out of range");
    if ((w >> (levels - 1)) < TRACK_MIN_LEVEL_EDGE || (h >> (levels - 1)) < TRACK_MIN_LEVEL_EDGE)
        return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": the image is too small for the pyramid levels requested");
    if (!(d->max_distance > 0.0f)) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": max_distance must be > 0");
    const double* intr = d->intrinsics4; const double* dist = d->distortion5;
    if (int rc = m.ready(d->use_context_camera != 0, intr, dist)) return rc;
    if (int rc = ensure_bricks(m)) return rc;
    if (s.photo()) {
        if (!m.cast_intensity) return m.fail(I3D_ERR_STATE, fn + ": this model has no intensity");
        if (int rc = m.intensity_ready()) return rc;
    }
    if (!d->use_context_camera) if (int rc = m.check_focal(intr)) return rc;
    s.cam0 = camera_of(intr, dist, w, h);
    s.levels = levels;
    size_t total = 0;
    for (int l = 0; l < levels; ++l) {
        level_size(w, h, l, s.lw[l], s.lh[l]);      // the keyframe pyramids' level sizes
        s.pyr_off[l] = total; total += (size_t)s.lw[l] * s.lh[l];
    }
    const size_t px = (size_t)w * h;
    MODEL_HIP(m, b.pyr.alloc(total));
    MODEL_HIP(m, b.vn.alloc(6 * px));
    MODEL_HIP(m, b.model.alloc((s.photo() ? 5 : 4) * px));
    MODEL_HIP(m, b.slab.alloc((size_t)track_assoc_rows(w, h) * TRACK_COLS));
    MODEL_HIP(m, b.state.alloc(1));
    MODEL_HIP(m, b.rstats.alloc(1));
    MODEL_HIP(m, hipMemcpyAsync(b.pyr.p, depth, px * sizeof(float), hipMemcpyHostToDevice, st));
    for (int l = 1; l < levels; ++l)                       // the valid-mean levels of the keyframes (Pyramid::downsampleDepth)
        launch_depth_down(st, s.lw[l - 1], b.pyr.p + s.pyr_off[l - 1], s.lw[l], s.lh[l], b.pyr.p + s.pyr_off[l]);
    if (rgbd) {                                            // the keyframes' luminance levels (Pyramid: pyrDown)
        MODEL_HIP(m, b.lum.alloc(total));
        MODEL_HIP(m, hipMemcpyAsync(b.lum.p, rgbd->luminance, px * sizeof(float), hipMemcpyHostToDevice, st));
        for (int l = 1; l < levels; ++l)
            launch_pyr_down(st, s.lw[l - 1], s.lh[l - 1], b.lum.p + s.pyr_off[l - 1], s.lw[l], s.lh[l], b.lum.p + s.pyr_off[l]);
    }
    MODEL_HIP(m, hipGetLastError());
    return I3D_OK;
}

PinholeCam level_cam(const Setup& s, int l) { return camera_at_level(s.cam0, l, s.lw[l], s.lh[l]); }

// the model planes of level l ray-cast at `ref` and the frame points of that level; planes in b.model / b.vn
int prepare_level(const Model& m, const i3d_track_desc* d, const Setup& s, int l, const TrackRef& ref) {
    hipStream_t st = m.stream; TrackBuffers& b = m.buf.track;
    const PinholeCam k = level_cam(s, l);
    const size_t px = (size_t)k.w * k.h;
    RenderCam rc; std::memset(&rc, 0, sizeof(rc));
    for (int i = 0; i < 9; ++i) rc.R[i] = ref.R[i];
    for (int a = 0; a < 3; ++a) rc.eye[a] = ref.eye[a];
    rc.k = k;
    rc.tmin = 0.0; rc.tmax = std::numeric_limits<double>::infinity();
    float* model = b.model.p;
    RenderPlanes out{model, model + px, nullptr, nullptr, s.photo() ? model + 4 * px : nullptr, nullptr, nullptr, s.photo() ? 1 : 0};
    MODEL_HIP(m, hipMemsetAsync(b.rstats.p, 0, sizeof(RenderStatsDev), st));
    m.cast(rc, out, b.rstats.p);
    launch_track_points(st, k, b.pyr.p + s.pyr_off[l], d->min_depth, d->max_depth, b.vn.p, b.vn.p + 3 * px);
    MODEL_HIP(m, hipGetLastError());
    return I3D_OK;
}

void launch_pass(hipStream_t st, TrackBuffers& b, const i3d_track_desc* d, const Setup& s, int l, const TrackRef& ref, int check_done) {
    const PinholeCam k = level_cam(s, l);
    const size_t px = (size_t)k.w * k.h;
    TrackPhoto ph{};
    if (s.rgbd) {
        const double wg = s.rgbd->geometric_weight, wp = s.rgbd->photo_weight;
        ph = TrackPhoto{b.lum.p + s.pyr_off[l], s.photo() ? b.model.p + 4 * px : nullptr, wg * wg, wp * wp, (double)d->max_distance, (double)s.rgbd->max_photo_residual};
    }
    launch_track_assoc(st, k, ref, b.vn.p, b.vn.p + 3 * px, b.model.p, b.model.p + px, s.rgbd ? &ph : nullptr, (double)d->max_distance, (double)d->min_normal_dot,
                       b.state.p, check_done, b.slab.p);
}

TrackState fresh_state(const Pose& P) {
    TrackState h; std::memset(&h, 0, sizeof(h));
    for (int i = 0; i < 9; ++i) h.R[i] = P.R[i];
    for (int a = 0; a < 3; ++a) h.t[a] = P.t[a];
    h.status = 1; h.first = 1;
    return h;
}

}  // namespace

extern "C" void i3d_track_desc_default(i3d_track_desc* d) {
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    d->levels = 1;                               // coarser levels widen the basin but bias the start of level 0
    d->iterations[0] = 30; d->iterations[1] = 10; d->iterations[2] = 10; d->iterations[3] = 10;
    d->use_refined_sdf = 1;
    d->use_context_camera = 1;
    d->max_distance = 0.05f;
    d->min_normal_dot = 0.8f;
    d->stop_rotation = 1e-6;
    d->stop_translation = 1e-6;
}

namespace i3d {

int track_frame_run(const Model& m, const i3d_track_desc* d, int32_t w, int32_t h, const float* depth, double* pose6_io, i3d_track_stats* stats, TrackRgbd* rgbd) {
    Setup s;
    if (int rc = setup(m, d, w, h, depth, d ? d->levels : 1, rgbd, s)) return rc;
    hipStream_t st = m.stream; TrackBuffers& b = m.buf.track;
    const double stop_r = d->stop_rotation, stop_t = d->stop_translation;
    i3d_track_stats out; std::memset(&out, 0, sizeof(out));
    out.status = 1;
    Pose P = pose_from_vec6(pose6_io);
    TrackState hs = fresh_state(P);
    TrackRef ref0{};                                        // the pose of the finest level's ray cast
    bool level0_ready = false;
    for (int l = s.levels - 1; l >= 0 && out.status != 3; --l) {
        const int budget = d->iterations[l];
        if (budget == 0 && l > 0) continue;
        if (budget == 0) {                                  // no iteration at the finest level: its planes for the final figures only
            ref0 = ref_from_pose(P);
            if (int rc = prepare_level(m, d, s, 0, ref0)) return rc;
            level0_ready = true;
            break;
        }
        // passes: each ray-casts the model at the current pose and iterates until the step is below the stop rule or the level's budget is used; a pass
        // that converges on its first step ends the level (the cast was taken at the pose it confirms)
        const int rows = track_assoc_rows(s.lw[l], s.lh[l]);
        int used = 0, level_status = 1;
        bool first_pass = true;
        while (used < budget) {
            const TrackRef ref = ref_from_pose(P);
            if (int rc = prepare_level(m, d, s, l, ref)) return rc;
            if (l == 0) { ref0 = ref; level0_ready = true; }
            const double ratio = hs.min_pivot_ratio;
            hs = fresh_state(P); hs.min_pivot_ratio = ratio;
            MODEL_HIP(m, hipMemcpyAsync(b.state.p, &hs, sizeof(hs), hipMemcpyHostToDevice, st));
            for (int it = used; it < budget; ++it) {        // back to back; a finished pass's remaining launches return at once (state->done)
                launch_pass(st, b, d, s, l, ref, 1);
                launch_track_solve(st, b.state.p, b.slab.p, 1, rows, 0, s.count_col(), stop_r, stop_t);
            }
            MODEL_HIP(m, hipGetLastError());
            MODEL_HIP(m, hipMemcpyAsync(&hs, b.state.p, sizeof(hs), hipMemcpyDeviceToHost, st));
            MODEL_HIP(m, hipStreamSynchronize(st));          // one synchronisation per pass
            used += hs.iters;
            out.iterations[l] = used;
            out.min_pivot_ratio = hs.min_pivot_ratio;
            if (l == 0 && first_pass) { out.rms_initial = hs.rms_first; if (rgbd) rgbd->photo_rms_initial = hs.rms_first_photo; }
            first_pass = false;
            if (hs.status == 2) {                           // too few inliers: the pose is left as it came in
                out.status = 2;
                out.valid_pixels = (int64_t)hs.sums[TRACK_SUMS]; out.inliers = (int64_t)hs.sums[28];
                if (rgbd) rgbd->photo_samples = (int64_t)hs.sums[TRACK_COL_PHOTO_N];
                if (stats) *stats = out;
                return I3D_OK;
            }
            for (int i = 0; i < 9; ++i) P.R[i] = hs.R[i];
            for (int a = 0; a < 3; ++a) P.t[a] = hs.t[a];
            if (hs.status == 3) { level_status = 3; break; } // degenerate: the last good estimate
            if (hs.status == 1) { level_status = 1; break; } // the budget is used
            level_status = 0;
            if (hs.iters <= 1) break;
        }
        out.status = level_status;
    }
    if (!level0_ready) {                                    // a degenerate coarser level ended the loop: cast the finest level for the final figures
        ref0 = ref_from_pose(P);
        if (int rc = prepare_level(m, d, s, 0, ref0)) return rc;
    }
    // the figures at the returned pose: one association pass against the finest level's ray cast, totals only
    TrackState e = fresh_state(P);
    MODEL_HIP(m, hipMemcpyAsync(b.state.p, &e, sizeof(e), hipMemcpyHostToDevice, st));
    launch_pass(st, b, d, s, 0, ref0, 0);
    launch_track_solve(st, b.state.p, b.slab.p, 1, track_assoc_rows(w, h), 1, s.count_col(), stop_r, stop_t);
    MODEL_HIP(m, hipGetLastError());
    MODEL_HIP(m, hipMemcpyAsync(&e, b.state.p, sizeof(e), hipMemcpyDeviceToHost, st));
    MODEL_HIP(m, hipStreamSynchronize(st));
    out.valid_pixels = (int64_t)e.sums[TRACK_SUMS]; out.inliers = (int64_t)e.sums[28];
    out.rms_final = e.sums[28] > 0.0 ? std::sqrt(e.sums[27] / e.sums[28]) : 0.0;
    if (rgbd) { rgbd->photo_samples = (int64_t)e.sums[TRACK_COL_PHOTO_N]; rgbd->photo_rms_final = rms_of(e.sums[TRACK_COL_PHOTO_SQ], e.sums[TRACK_COL_PHOTO_N]); }
    vec6_from_pose(P, pose6_io);
    if (stats) *stats = out;
    return I3D_OK;
}

int track_sums_run(const Model& m, const i3d_track_desc* d, int32_t w, int32_t h, const float* depth, int32_t level, const double* pose_ref6, const double* pose_cur6,
                   double* sums, int64_t* inliers, TrackRgbd* rgbd) {
    Setup s;
    if (int rc = setup(m, d, w, h, depth, level + 1, rgbd, s)) return rc;
    hipStream_t st = m.stream; TrackBuffers& b = m.buf.track;
    TrackRef ref;                                           // exactly the renderer's camera of pose_ref6 (render.cpp), t as given
    {
        FrameConst fc; fm::frame_from_pose(pose_ref6, fc);
        for (int i = 0; i < 9; ++i) ref.R[i] = fc.hot.R[i];
        for (int a = 0; a < 3; ++a) { ref.t[a] = pose_ref6[3 + a]; ref.eye[a] = -((fc.hot.R[a] * fc.hot.t[0] + fc.hot.R[3 + a] * fc.hot.t[1]) + fc.hot.R[6 + a] * fc.hot.t[2]); }
    }
    if (int rc = prepare_level(m, d, s, level, ref)) return rc;
    TrackState e = fresh_state(pose_from_vec6(pose_cur6));
    MODEL_HIP(m, hipMemcpyAsync(b.state.p, &e, sizeof(e), hipMemcpyHostToDevice, st));
    launch_pass(st, b, d, s, level, ref, 0);
    launch_track_solve(st, b.state.p, b.slab.p, 1, track_assoc_rows(s.lw[level], s.lh[level]), 1, s.count_col(), 0.0, 0.0);
    MODEL_HIP(m, hipGetLastError());
    MODEL_HIP(m, hipMemcpyAsync(&e, b.state.p, sizeof(e), hipMemcpyDeviceToHost, st));
    MODEL_HIP(m, hipStreamSynchronize(st));
    for (int k = 0; k < TRACK_SUMS; ++k) sums[k] = e.sums[k];
    if (inliers) *inliers = (int64_t)e.sums[28];
    if (rgbd) { sums[29] = e.sums[TRACK_COL_PHOTO_SQ]; sums[30] = e.sums[TRACK_COL_PHOTO_N]; rgbd->photo_samples = (int64_t)e.sums[TRACK_COL_PHOTO_N]; }
    return I3D_OK;
}

}  // namespace i3d

extern "C" int i3d_track_frame(i3d_context* c, const i3d_track_desc* d, int32_t w, int32_t h, const float* depth, double* pose6_io, i3d_track_stats* stats) {
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_track_frame: null context");
    if (!pose6_io) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_track_frame: null pose");
    return track_frame_run(ContextModel(c, "i3d_track_frame", d && d->use_refined_sdf != 0), d, w, h, depth, pose6_io, stats);
}

extern "C" int i3d_debug_track_sums(i3d_context* c, const i3d_track_desc* d, int32_t w, int32_t h, const float* depth, int32_t level, const double* pose_ref6,
                                    const double* pose_cur6, double* sums29, int64_t* inliers) {
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_debug_track_sums: null context");
    if (!pose_ref6 || !pose_cur6 || !sums29) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_debug_track_sums: null argument");
    if (d && (level < 0 || level >= d->levels)) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_debug_track_sums: level out of range");
    return track_sums_run(ContextModel(c, "i3d_debug_track_sums", d && d->use_refined_sdf != 0), d, w, h, depth, level, pose_ref6, pose_cur6, sums29, inliers);
}

extern "C" void i3d_track_rgbd_desc_default(i3d_track_rgbd_desc* d) {
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    i3d_track_desc_default(&d->base);
    d->geometric_weight = 1.0;
    d->photo_weight = 0.1;                       // metres per unit luminance (the sweep behind it)
    d->max_photo_residual = 0.0f;                // open
}

extern "C" int i3d_track_frame_rgbd(i3d_context* c, const i3d_track_rgbd_desc* d, int32_t w, int32_t h, const float* depth, const float* luminance, double* pose6_io,
                                    i3d_track_rgbd_stats* stats) {
    const char* fn = "i3d_track_frame_rgbd";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null context");
    if (!d) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null descriptor");
    if (!pose6_io) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null pose");
    TrackRgbd r{luminance, d->geometric_weight, d->photo_weight, d->max_photo_residual};
    i3d_track_stats base; std::memset(&base, 0, sizeof(base));
    const int rc = track_frame_run(ContextModel(c, fn, d->base.use_refined_sdf != 0), &d->base, w, h, depth, pose6_io, &base, &r);
    if (rc == I3D_OK && stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->base = base; stats->photo_samples = r.photo_samples; stats->photo_rms_initial = r.photo_rms_initial; stats->photo_rms_final = r.photo_rms_final;
    }
    return rc;
}

extern "C" int i3d_debug_track_rgbd_sums(i3d_context* c, const i3d_track_rgbd_desc* d, int32_t w, int32_t h, const float* depth, const float* luminance, int32_t level,
                                         const double* pose_ref6, const double* pose_cur6, double* sums31, int64_t* inliers, int64_t* photo_samples) {
    const char* fn = "i3d_debug_track_rgbd_sums";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null context");
    if (!d || !pose_ref6 || !pose_cur6 || !sums31) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null argument");
    if (level < 0 || level >= d->base.levels) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": level out of range");
    TrackRgbd r{luminance, d->geometric_weight, d->photo_weight, d->max_photo_residual};
    const int rc = track_sums_run(ContextModel(c, fn, d->base.use_refined_sdf != 0), &d->base, w, h, depth, level, pose_ref6, pose_cur6, sums31, inliers, &r);
    if (rc == I3D_OK && photo_samples) *photo_samples = r.photo_samples;
    return rc;
}
