// Keyframes and camera: the two keyframe uploads (pyramids from the caller, or built on the device from level-0 colour + depth), one pyramid image back,
// resizeDepth, and the camera pair.
#include "context.hpp"
#include "../device/level_kernels.hpp"

using namespace i3d;

// what both keyframe uploads do around their images: drop the old keyframe state and size the tables for K keyframes of `levels` levels ...
static void reset_frames(i3d_context* c, int K, int levels) {
    c->have_frames = false; c->K = K; c->levels = levels; c->cull_level = -1;
    c->slots = 0; c->assembled = false;            // K sizes the camera blocks and solver vectors: force alloc_rows() to run again
    c->fw.resize(levels); c->fh.resize(levels);
    c->lum.clear(); c->depth.clear(); c->bgr.clear();
    c->lum.resize((size_t)K * levels); c->depth.resize((size_t)K * levels); c->bgr.resize((size_t)K * levels);
}
// ... and, with every image queued: the keyframe constants' storage, the end of the uploads, and a camera only if the keyframe count is the one it was set for
static int finish_frames(i3d_context* c) {
    CTX_HIP(c, c->d_frames.alloc(c->K)); CTX_HIP(c, c->d_frames_cand.alloc(c->K));
    CTX_HIP(c, ctx_sync(c));
    c->have_frames = true;
    if ((int)c->poses.size() != 6 * c->K) { c->poses.assign((size_t)6 * c->K, 0.0); c->have_camera = false; }
    return I3D_OK;
}

extern "C" {

int i3d_set_frames(i3d_context* c, int32_t K, int32_t levels, const int32_t* widths, const int32_t* heights,
                   const float* const* lum, const float* const* depth, const uint8_t* const* bgr) {
    CTX_ENTER(c, K > 0 && levels > 0 && widths && heights && lum && depth, ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_set_frames: bad arguments"));
    reset_frames(c, K, levels);
    c->fw.assign(widths, widths + levels); c->fh.assign(heights, heights + levels);
    for (int f = 0; f < K; ++f) for (int l = 0; l < levels; ++l) {
        const size_t k = (size_t)f * levels + l, px = (size_t)widths[l] * heights[l];
        if (!lum[k] || !depth[k]) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_set_frames: null image");
        CTX_HIP(c, c->lum[k].alloc(px + 4));       /* + 16 B: the 16-byte tap loads of the cost kernels may run past the last row of an image narrower than 4 pixels (build.hip) */ CTX_HIP(c, c->depth[k].alloc(px));
        CTX_HIP(c, ctx_upload(c, c->lum[k].p, lum[k], px));
        CTX_HIP(c, ctx_upload(c, c->depth[k].p, depth[k], px));
        if (bgr && bgr[k]) { CTX_HIP(c, c->bgr[k].alloc(px * 3)); CTX_HIP(c, ctx_upload(c, c->bgr[k].p, bgr[k], px * 3)); }
    }
    return finish_frames(c);
}

// Intrinsic3D::init's per-keyframe Pyramid(num_rgbd_levels, color, depth) (intrinsic3d.cpp:182-187, rgbd/pyramid.cpp:59-166) on the device:
// level-0 colour + depth in, float luminance / depth pyramids out (colour is kept at level 0 only: recomputeColors reads nothing else)
int i3d_set_frames_rgbd(i3d_context* c, int32_t K, int32_t levels, int32_t width, int32_t height, const uint8_t* const* bgr, const float* const* depth) {
    CTX_ENTER(c, K > 0 && levels > 0 && width > 0 && height > 0 && bgr && depth, ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_set_frames_rgbd: bad arguments"));
    if ((width >> (levels - 1)) < 1 || (height >> (levels - 1)) < 1) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_set_frames_rgbd: more levels than the image size allows");
    hipStream_t st = c->stream;
    reset_frames(c, K, levels);
    for (int l = 0; l < levels; ++l) level_size(width, height, l, c->fw[l], c->fh[l]);
    for (int f = 0; f < K; ++f) {
        if (!bgr[f] || !depth[f]) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_set_frames_rgbd: null image");
        const size_t k0 = (size_t)f * levels, px = (size_t)width * height;
        CTX_HIP(c, c->bgr[k0].alloc(px * 3)); CTX_HIP(c, c->lum[k0].alloc(px + 4)); CTX_HIP(c, c->depth[k0].alloc(px));
        CTX_HIP(c, ctx_upload(c, c->bgr[k0].p, bgr[f], px * 3));
        CTX_HIP(c, ctx_upload(c, c->depth[k0].p, depth[f], px));
        launch_lum_from_bgr(st, (int)px, c->bgr[k0].p, c->lum[k0].p);
        for (int l = 1; l < levels; ++l) {
            const size_t k = k0 + l, n = (size_t)c->fw[l] * c->fh[l];
            CTX_HIP(c, c->lum[k].alloc(n + 4)); CTX_HIP(c, c->depth[k].alloc(n));
            launch_pyr_down(st, c->fw[l - 1], c->fh[l - 1], c->lum[k - 1].p, c->fw[l], c->fh[l], c->lum[k].p);
            launch_depth_down(st, c->fw[l - 1], c->depth[k - 1].p, c->fw[l], c->fh[l], c->depth[k].p);
        }
    }
    CTX_HIP(c, hipGetLastError());
    return finish_frames(c);
}
// resizeDepth(depth camera, depth, colour camera) (rgbd/processing.cpp:129-181), called per keyframe by Intrinsic3D::init (intrinsic3d.cpp:182-184)
// before the pyramid is built; intrinsics are (fx, fy, cx, cy) as floats.  Same size in and out: a plain copy, like the reference.
int i3d_resize_depth(int32_t device_ordinal, int32_t in_w, int32_t in_h, const float* depth_in, const float* in_intr, int32_t out_w, int32_t out_h,
                     const float* out_intr, float* depth_out) {
    if (!depth_in || !depth_out || !in_intr || !out_intr || in_w <= 0 || in_h <= 0 || out_w <= 0 || out_h <= 0) return I3D_ERR_INVALID_ARGUMENT;
    if (in_w == out_w && in_h == out_h) { std::memcpy(depth_out, depth_in, sizeof(float) * (size_t)in_w * in_h); return I3D_OK; }
    int ndev = 0; if (hipGetDeviceCount(&ndev) != hipSuccess || device_ordinal < 0 || device_ordinal >= ndev) return I3D_ERR_NO_DEVICE;
    if (hipSetDevice(device_ordinal) != hipSuccess) return I3D_ERR_HIP;
    DevBuf<float> a, b;
    if (a.alloc((size_t)in_w * in_h) != hipSuccess || b.alloc((size_t)out_w * out_h) != hipSuccess) return I3D_ERR_HIP;
    if (hipMemcpy(a.p, depth_in, sizeof(float) * (size_t)in_w * in_h, hipMemcpyHostToDevice) != hipSuccess) return I3D_ERR_HIP;
    launch_resize_depth(nullptr, in_w, in_h, a.p, in_intr, out_w, out_h, out_intr, b.p);
    if (hipMemcpy(depth_out, b.p, sizeof(float) * (size_t)out_w * out_h, hipMemcpyDeviceToHost) != hipSuccess) return I3D_ERR_HIP;
    return hipGetLastError() == hipSuccess ? I3D_OK : I3D_ERR_HIP;
}
// one pyramid image back to the host (parity probe / callers that still want the images)
int i3d_get_frame_image(i3d_context* c, int32_t frame, int32_t level, float* lum, float* depth) {
    CTX_ENTER(c, c->have_frames && frame >= 0 && frame < c->K && level >= 0 && level < c->levels, ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_get_frame_image: bad frame / level"));
    const size_t k = (size_t)frame * c->levels + level, n = (size_t)c->fw[level] * c->fh[level];
    if (lum) CTX_HIP(c, ctx_download(c, lum, c->lum[k].p, n));
    if (depth) CTX_HIP(c, ctx_download(c, depth, c->depth[k].p, n));
    CTX_HIP(c, ctx_sync(c));
    return I3D_OK;
}

int i3d_set_camera(i3d_context* c, const double* intr, const double* dist, const double* poses) {
    CTX_ENTER(c, intr && dist && poses, ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_set_camera: null pointer"));
    if (!c->have_frames) return ctx_fail(c, I3D_ERR_STATE, "i3d_set_camera: set the keyframes first");
    std::memcpy(c->intr, intr, sizeof(double) * 4); std::memcpy(c->dist, dist, sizeof(double) * 5);
    c->poses.assign(poses, poses + (size_t)6 * c->K);
    c->have_camera = true;
    return I3D_OK;
}
int i3d_get_camera(i3d_context* c, double* intr, double* dist, double* poses) {
    CTX_ENTER(c, c->have_camera, ctx_fail(c, I3D_ERR_STATE, "i3d_get_camera: no camera"));
    if (intr) std::memcpy(intr, c->intr, sizeof(double) * 4);
    if (dist) std::memcpy(dist, c->dist, sizeof(double) * 5);
    if (poses) std::memcpy(poses, c->poses.data(), sizeof(double) * 6 * (size_t)c->K);
    return I3D_OK;
}

}  // extern "C"
