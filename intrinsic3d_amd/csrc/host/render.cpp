// The ray cast of a model into a camera view (render_kernels.hip): the fp64 camera of the view and render_run, the driver for every model (the context here,
// the fusion volume in fusion.cpp), then i3d_render_view and i3d_render_view_color: their validation and their choice of camera.
// Reads the grid, SH, stored colour, camera and keyframe images; writes only the model's buffers (bitmap, output planes, stats), nothing the optimiser reads.
#include "context.hpp"
#include "../device/frame_math.hpp"
#include <limits>

using namespace i3d;

namespace i3d {

RenderCam render_cam(const PinholeCam& k, const double* pose6, float min_depth, float max_depth) {
    RenderCam cam; std::memset(&cam, 0, sizeof(cam));
    cam.k = k;
    FrameConst fc; fm::frame_from_pose(pose6, fc);
    for (int i = 0; i < 9; ++i) cam.R[i] = fc.hot.R[i];
    for (int a = 0; a < 3; ++a) cam.eye[a] = -((fc.hot.R[a] * fc.hot.t[0] + fc.hot.R[3 + a] * fc.hot.t[1]) + fc.hot.R[6 + a] * fc.hot.t[2]);
    cam.tmin = min_depth > 0.0f ? (double)min_depth : 0.0;
    cam.tmax = max_depth > 0.0f ? (double)max_depth : std::numeric_limits<double>::infinity();
    return cam;
}

int render_run(const Model& m, const RenderCam& cam, const RenderWant& w, const float* keyframe_lum, i3d_render_stats* stats) {
    if (int rc = m.make_current()) return rc;
    if (int rc = ensure_bricks(m)) return rc;
    hipStream_t st = m.stream;
    const size_t px = (size_t)cam.k.w * cam.k.h;
    size_t total = 0;                                // the scratch: the planes requested, one after the other
    auto take = [&total](const float* wanted, size_t n) { const size_t at = total; if (wanted) total += n; return at; };
    float* const color = w.colour_view ? w.color : nullptr;
    const size_t o_depth = take(w.depth, px), o_normal = take(w.normal, 3 * px), o_albedo = take(w.albedo, px), o_shading = take(w.shading, px),
                 o_intensity = take(w.intensity, px), o_residual = take(w.residual, px), o_color = take(color, 3 * px);
    if (total) MODEL_HIP(m, m.buf.planes.alloc(total));
    MODEL_HIP(m, m.buf.stats.alloc(1));
    float* base = m.buf.planes.p;
    const RenderPlanes out{w.depth ? base + o_depth : nullptr, w.normal ? base + o_normal : nullptr, w.albedo ? base + o_albedo : nullptr,
                           w.shading ? base + o_shading : nullptr, w.intensity ? base + o_intensity : nullptr, w.residual ? base + o_residual : nullptr,
                           w.residual ? keyframe_lum : nullptr, w.shading || w.intensity || w.residual ? 1 : 0};
    const RenderColorPlanes cplanes{out.depth, color ? base + o_color : nullptr};
    MODEL_HIP(m, hipMemsetAsync(m.buf.stats.p, 0, sizeof(RenderStatsDev), st));
    if (w.colour_view) m.cast_color(cam, cplanes, m.buf.stats.p);
    else m.cast(cam, out, m.buf.stats.p);
    MODEL_HIP(m, hipGetLastError());
    auto back = [&](float* dst, const float* src, size_t n) -> hipError_t { return dst ? hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToHost, st) : hipSuccess; };
    MODEL_HIP(m, back(w.depth, out.depth, px)); MODEL_HIP(m, back(w.normal, out.normal, 3 * px)); MODEL_HIP(m, back(w.albedo, out.albedo, px));
    MODEL_HIP(m, back(w.shading, out.shading, px)); MODEL_HIP(m, back(w.intensity, out.intensity, px)); MODEL_HIP(m, back(w.residual, out.residual, px));
    MODEL_HIP(m, back(color, cplanes.color, 3 * px));
    RenderStatsDev s{};
    MODEL_HIP(m, hipMemcpyAsync(&s, m.buf.stats.p, sizeof(s), hipMemcpyDeviceToHost, st));
    MODEL_HIP(m, hipStreamSynchronize(st));
    if (stats) { stats->hits = (int64_t)s.hits; stats->samples = (int64_t)s.samples; stats->residual_sq_sum = w.residual ? s.residual_sq : 0.0; }
    return I3D_OK;
}

}  // namespace i3d

// the camera of a view of the context, after the state check: a keyframe's (its refined pose, the intrinsics at the level) or the descriptor's own.  residual: the
// residual plane is asked for, which a free camera cannot serve
static int view_camera(const ContextModel& m, const i3d_render_desc* d, bool residual, PinholeCam& k, const double*& pose) {
    constexpr int RENDER_MAX_EDGE = 1 << 15;
    const i3d_context* c = m.c;
    if (d->frame >= 0) {
        if (!c->have_frames) return m.fail(I3D_ERR_STATE, m.fn + ": no keyframes");
        if (!c->have_camera) return m.fail(I3D_ERR_STATE, m.fn + ": no camera");
        if (d->frame >= c->K || d->level < 0 || d->level >= c->levels) return m.fail(I3D_ERR_INVALID_ARGUMENT, m.fn + ": frame / level out of range");
        k = camera_at_level(camera_of(c->intr, c->dist, c->fw[0], c->fh[0]), d->level, c->fw[d->level], c->fh[d->level]);
        pose = c->poses.data() + (size_t)6 * d->frame;
    } else {
        if (residual) return m.fail(I3D_ERR_INVALID_ARGUMENT, m.fn + ": a residual needs a keyframe (frame >= 0)");
        if (d->width <= 0 || d->height <= 0 || d->width > RENDER_MAX_EDGE || d->height > RENDER_MAX_EDGE)
            return m.fail(I3D_ERR_INVALID_ARGUMENT, m.fn + ": image size out of range");
        k = camera_of(d->intrinsics4, d->distortion5, d->width, d->height);
        pose = d->pose6;
    }
    return I3D_OK;
}

extern "C" int i3d_render_view(i3d_context* c, const i3d_render_desc* d, float* depth, float* normal, float* albedo, float* shading, float* intensity,
                               float* residual, i3d_render_stats* stats) {
    if (!c || !d) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_render_view: null argument");
    const ContextModel m(c, "i3d_render_view", d->use_refined_sdf != 0);
    if (int rc = m.check_field()) return rc;
    PinholeCam k; const double* pose = nullptr;
    if (int rc = view_camera(m, d, residual != nullptr, k, pose)) return rc;
    if ((shading || intensity || residual) && !c->have_sh)
        return m.fail(I3D_ERR_STATE, m.fn + ": shading, intensity and residual need the per-voxel SH (i3d_set_voxel_sh / i3d_estimate_sh)");
    return render_run(m, render_cam(k, pose, d->min_depth, d->max_depth), RenderWant{depth, normal, albedo, shading, intensity, residual},
                      residual ? c->lum[(size_t)d->frame * c->levels + d->level].p : nullptr, stats);
}

// the colour view: the camera of i3d_render_view, depth and the stored colour; no SH is read
extern "C" int i3d_render_view_color(i3d_context* c, const i3d_render_desc* d, float* color, float* depth, i3d_render_stats* stats) {
    if (!c || !d) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_render_view_color: null argument");
    const ContextModel m(c, "i3d_render_view_color", d->use_refined_sdf != 0);
    if (int rc = m.check_field()) return rc;
    PinholeCam k; const double* pose = nullptr;
    if (int rc = view_camera(m, d, false, k, pose)) return rc;
    return render_run(m, render_cam(k, pose, d->min_depth, d->max_depth), RenderWant{depth, nullptr, nullptr, nullptr, nullptr, nullptr, color, true}, nullptr, stats);
}
