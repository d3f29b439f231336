// i3d_render_view: validation, the fp64 camera of the view, the cached brick bitmap and the one launch of k_render (render_kernels.hip).
// Reads the grid, SH, camera and keyframe images; writes only its own buffers (bitmap, output planes, stats), nothing the optimiser reads.
#include "context.hpp"
#include "../device/frame_math.hpp"
#include <climits>
#include <limits>

using namespace i3d;

namespace {

constexpr int RENDER_PLANES = 8;                 // depth | normal x3 | albedo | shading | intensity | residual
constexpr int RENDER_MAX_EDGE = 1 << 15;

}  // namespace

namespace i3d {

// the brick bitmap of the current grid: bounds of the bricks that hold a voxel with weight != 0, then one bit per brick of that box.  Built on first use after
// set_grid_device (every change of the stored voxels goes through it and drops the cache).
int render_ensure_bricks(i3d_context* c) {
    if (c->render_bricks_ok) return I3D_OK;
    hipStream_t st = c->stream;
    const int init[6] = {INT_MAX, INT_MAX, INT_MAX, INT_MIN, INT_MIN, INT_MIN};
    int b[6];
    CTX_HIP(c, c->render_bounds.alloc(6));
    CTX_HIP(c, hipMemcpyAsync(c->render_bounds.p, init, sizeof(init), hipMemcpyHostToDevice, st));
    launch_render_brick_bounds(st, c->N, c->cx.p, c->cy.p, c->cz.p, c->weight.p, c->render_bounds.p);
    CTX_HIP(c, hipGetLastError());
    CTX_HIP(c, hipMemcpyAsync(b, c->render_bounds.p, sizeof(b), hipMemcpyDeviceToHost, st));
    CTX_HIP(c, hipStreamSynchronize(st));
    for (int a = 0; a < 3; ++a) { c->render_lo[a] = 0; c->render_dim[a] = 0; }
    if (b[0] <= b[3]) {                          // else no voxel has a weight: the box is empty and every ray misses
        long long bits = 1;
        for (int a = 0; a < 3; ++a) { c->render_lo[a] = b[a]; c->render_dim[a] = b[3 + a] - b[a] + 1; bits *= c->render_dim[a]; }
        if (bits > (1ll << 31)) {
            for (int a = 0; a < 3; ++a) c->render_dim[a] = 0;
            return ctx_fail(c, I3D_ERR_CAPACITY, "i3d_render_view: the brick bitmap of the grid's bounding box would exceed 2^31 bits (" + std::to_string(bits) + ")");
        }
        const size_t words = (size_t)((bits + 31) / 32);
        CTX_HIP(c, c->render_bits.alloc(words));
        CTX_HIP(c, hipMemsetAsync(c->render_bits.p, 0, words * sizeof(unsigned), st));
        launch_render_brick_fill(st, c->N, c->cx.p, c->cy.p, c->cz.p, c->weight.p, c->render_bits.p, c->render_lo, c->render_dim);
        CTX_HIP(c, hipGetLastError());
    }
    c->render_bricks_ok = true;
    return I3D_OK;
}

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

RenderGrid render_grid(const i3d_context* c, bool refined) {
    return RenderGrid{HashTable{c->hkeys.p, c->hvals.p, c->hmask}, c->nbr.p, c->N, c->weight.p, refined ? c->x_sdf.p : c->sdf0.p, c->x_alb.p, c->sh.p,
                      (double)c->voxel_size, c->render_bits.p, {c->render_lo[0], c->render_lo[1], c->render_lo[2]}, {c->render_dim[0], c->render_dim[1], c->render_dim[2]}};
}

}  // namespace i3d

extern "C" int i3d_render_view(i3d_context* c, const i3d_render_desc* d, float* depth, float* normal, float* albedo, float* shading, float* intensity,
                               float* residual, i3d_render_stats* stats) {
    if (!c || !d) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_render_view: null argument");
    if (!c->have_grid) return ctx_fail(c, I3D_ERR_STATE, "i3d_render_view: no grid");
    const bool need_sh = shading || intensity || residual;
    PinholeCam k; const double* pose = nullptr;
    if (d->frame >= 0) {
        if (!c->have_frames) return ctx_fail(c, I3D_ERR_STATE, "i3d_render_view: no keyframes");
        if (!c->have_camera) return ctx_fail(c, I3D_ERR_STATE, "i3d_render_view: no camera");
        if (d->frame >= c->K || d->level < 0 || d->level >= c->levels) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_render_view: frame / level out of range");
        k = camera_at_level(camera_of(c->intr, c->dist, c->fw[0], c->fh[0]), d->level, c->fw[d->level], c->fh[d->level]);
        pose = c->poses.data() + (size_t)6 * d->frame;
    } else {
        if (residual) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_render_view: a residual needs a keyframe (frame >= 0)");
        if (d->width <= 0 || d->height <= 0 || d->width > RENDER_MAX_EDGE || d->height > RENDER_MAX_EDGE)
            return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_render_view: image size out of range");
        k = camera_of(d->intrinsics4, d->distortion5, d->width, d->height);
        pose = d->pose6;
    }
    if (need_sh && !c->have_sh) return ctx_fail(c, I3D_ERR_STATE, "i3d_render_view: shading, intensity and residual need the per-voxel SH (i3d_set_voxel_sh / i3d_estimate_sh)");
    const RenderCam cam = render_cam(k, pose, d->min_depth, d->max_depth);

    CTX_HIP(c, hipSetDevice(c->device));
    if (int rc = render_ensure_bricks(c)) return rc;
    hipStream_t st = c->stream;
    const size_t px = (size_t)k.w * k.h;
    const bool any_plane = depth || normal || albedo || need_sh;
    if (any_plane) CTX_HIP(c, c->render_planes.alloc(RENDER_PLANES * px));
    CTX_HIP(c, c->render_stats.alloc(1));
    float* base = c->render_planes.p;
    RenderPlanes out{depth ? base : nullptr, normal ? base + px : nullptr, albedo ? base + 4 * px : nullptr, shading ? base + 5 * px : nullptr,
                     intensity ? base + 6 * px : nullptr, residual ? base + 7 * px : nullptr,
                     residual ? c->lum[(size_t)d->frame * c->levels + d->level].p : nullptr, need_sh ? 1 : 0};
    const RenderGrid g = render_grid(c, d->use_refined_sdf != 0);
    CTX_HIP(c, hipMemsetAsync(c->render_stats.p, 0, sizeof(RenderStatsDev), st));
    launch_render(st, g, cam, out, c->render_stats.p);
    CTX_HIP(c, hipGetLastError());
    auto back = [&](float* dst, const float* src, size_t n) -> hipError_t { return dst ? hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToHost, st) : hipSuccess; };
    CTX_HIP(c, back(depth, out.depth, px)); CTX_HIP(c, back(normal, out.normal, 3 * px)); CTX_HIP(c, back(albedo, out.albedo, px));
    CTX_HIP(c, back(shading, out.shading, px)); CTX_HIP(c, back(intensity, out.intensity, px)); CTX_HIP(c, back(residual, out.residual, px));
    RenderStatsDev s{};
    CTX_HIP(c, hipMemcpyAsync(&s, c->render_stats.p, sizeof(s), hipMemcpyDeviceToHost, st));
    CTX_HIP(c, hipStreamSynchronize(st));
    if (stats) { stats->hits = (int64_t)s.hits; stats->samples = (int64_t)s.samples; stats->residual_sq_sum = s.residual_sq; }
    return I3D_OK;
}
