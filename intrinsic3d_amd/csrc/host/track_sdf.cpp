// Registration of depth frames on the stored field, no ray cast (track_sdf_kernels.hip; the definition is DESIGN.md section 19).
// track_sdf_chunks is the one driver for every model (model.hpp: the context here, the fusion volume in fusion.cpp) and every form: a chunk of frames at a time, the scratch
// layout, the upload, the pivot pass, the whole budget launched back to back with k_track_solve at one workgroup per frame, the figures at the returned poses; two
// stream synchronisations per chunk.  A pose comes in and goes out world -> camera, as i3d_track_frame's; the loop runs on its inverse, the camera -> world
// pose of section 18.  Reads the grid and, with use_context_camera, the context's camera; writes only the model's TrackSdfBuffers.
//   i3d_track_frame_sdf, i3d_fusion_track_sdf             track_sdf_run: the single frame's validation, then the driver with one frame
//   i3d_track_frames_sdf / i3d_track_keyframes_sdf         their own checks, then the driver with the frames uploaded / resident
//   the _rgbd forms, i3d_fusion_track_sdf_rgbd            (sections 21, 22) the same with a TrackSdfRgbd: the luminance beside the depth, the model's intensity
//                                                         volume filled once per call, the passes with the combined system, the usable count of the pivot pass
//   the i3d_debug_*_sums entry points                     the driver with a TrackSdfDebug: one pass of one frame at a given pivot
#include <algorithm>
#include "context.hpp"

using namespace i3d;

namespace {

constexpr int TRACK_SDF_MAX_EDGE = 1 << 15;
constexpr int TRACK_SDF_MAX_STRIDE = 16;
constexpr int TRACK_SDF_MAX_ITERATIONS = 200;

// the size and descriptor faults of section 19
int check_desc(const Model& m, const i3d_track_sdf_desc* d, int32_t w, int32_t h) {
    const std::string& fn = m.fn;
    if (w <= 0 || h <= 0 || w > TRACK_SDF_MAX_EDGE || h > TRACK_SDF_MAX_EDGE) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": image size out of range");
    if (d->stride < 1 || d->stride > TRACK_SDF_MAX_STRIDE) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": stride must be 1.." + std::to_string(TRACK_SDF_MAX_STRIDE));
    if (d->iterations < 0 || d->iterations > TRACK_SDF_MAX_ITERATIONS)
        return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": iterations must be 0.." + std::to_string(TRACK_SDF_MAX_ITERATIONS));
    if (!std::isfinite(d->max_distance) || !(d->max_distance > 0.0)) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": max_distance must be finite and > 0");
    if (!std::isfinite(d->huber_delta)) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": huber_delta must be finite (<= 0: off)");
    return I3D_OK;
}

// the faults of section 21.1 item 7 that the descriptor alone shows
int check_rgbd(const Model& m, const TrackSdfRgbd& r) {
    if (int rc = m.check_weights(r.geometric_weight, r.photo_weight)) return rc;
    if (!std::isfinite(r.max_photo_residual)) return m.fail(I3D_ERR_INVALID_ARGUMENT, m.fn + ": max_photo_residual must be finite (<= 0: open)");
    return I3D_OK;
}

TrackSdfPhoto photo_of(const TrackSdfRgbd& r, const double* vol) {
    return TrackSdfPhoto{vol, r.geometric_weight * r.geometric_weight, r.photo_weight * r.photo_weight, (double)r.max_photo_residual};
}

// the column whose total must reach TRACK_MIN_INLIERS: the photometric samples when there is no geometric term
int count_col_of(const TrackSdfRgbd* r) { return r && !(r->geometric_weight > 0.0) ? TRACK_COL_PHOTO_N : 28; }

// the kernels' parameters of a frame of w x h under the camera intr / dist
TrackSdfParams make_params(const i3d_track_sdf_desc* d, const double* intr, const double* dist, int32_t w, int32_t h, int row_cap) {
    TrackSdfParams prm; std::memset(&prm, 0, sizeof(prm));
    prm.cam = camera_of(intr, dist, w, h);
    const int ws = (w + d->stride - 1) / d->stride, hs_ = (h + d->stride - 1) / d->stride;
    const long long n = (long long)ws * hs_;
    prm.stride = d->stride; prm.ws = ws; prm.n = n;
    prm.min_depth = d->min_depth; prm.max_depth = d->max_depth;
    prm.max_distance = d->max_distance; prm.huber_delta = d->huber_delta;
    prm.per_lane = register_per_lane(n, row_cap);
    return prm;
}

// the figures of section 19.1 from the state after the figures pass, and the pose when a step was applied
// rgbd (section 21): the usable count is the pivot pass's, the status of a budget of 0 goes by the column that counts, and the photometric figures go to rstats
void finish_frame(const TrackState& hs, int budget, const double* c, double* pose6_io, i3d_track_sdf_stats* stats, const TrackSdfRgbd* rgbd = nullptr,
                  double usable = 0.0, i3d_track_sdf_rgbd_stats* rstats = nullptr) {
    i3d_track_sdf_stats out; std::memset(&out, 0, sizeof(out));
    out.valid_pixels = (int64_t)(rgbd ? usable : hs.sums[TRACK_SDF_COL_USABLE]); out.valid = (int64_t)hs.sums[TRACK_SUMS]; out.inliers = (int64_t)hs.sums[28];
    out.rms_final = rms_of(hs.sums[27], hs.sums[28]);
    out.rms_initial = budget > 0 ? hs.rms_first : out.rms_final;
    out.iterations = hs.iters;
    out.min_pivot_ratio = hs.min_pivot_ratio;
    out.status = budget > 0 ? hs.status : (hs.sums[count_col_of(rgbd)] < (double)TRACK_MIN_INLIERS ? 2 : 1);
    if (hs.iters > 0) {                                     // no step applied: the pose is left as it came in, bit for bit
        Pose Pn;
        for (int i = 0; i < 9; ++i) Pn.R[i] = hs.R[i];
        for (int a = 0; a < 3; ++a) Pn.t[a] = hs.t[a] + c[a];
        vec6_from_pose(Pn, pose6_io);
    }
    if (stats) *stats = out;
    if (rstats) {
        std::memset(rstats, 0, sizeof(*rstats));
        rstats->base = out;
        rstats->photo_samples = (int64_t)hs.sums[TRACK_COL_PHOTO_N];
        rstats->photo_rms_final = rms_of(hs.sums[TRACK_COL_PHOTO_SQ], hs.sums[TRACK_COL_PHOTO_N]);
        rstats->photo_rms_initial = budget > 0 ? hs.rms_first_photo : rstats->photo_rms_final;
    }
}

constexpr size_t TRACK_SDF_BATCH_BYTES = (size_t)512 << 20;     // the scratch of a chunk at most (a single frame may exceed it: a chunk holds at least one)
constexpr int TRACK_SDF_BATCH_MAX = 65535;                      // frames of a chunk at most: gridDim.y

// frames per chunk (section 20.3): the largest number whose scratch stays within TRACK_SDF_BATCH_BYTES, at least 1, at most TRACK_SDF_BATCH_MAX and max_chunk
int chunk_frames(size_t frame_bytes, int num, int max_chunk) {
    long long n = (long long)(TRACK_SDF_BATCH_BYTES / frame_bytes);
    n = std::max(1LL, std::min(n, (long long)TRACK_SDF_BATCH_MAX));
    if (max_chunk > 0) n = std::min(n, (long long)max_chunk);
    return (int)std::min(n, (long long)num);
}

}  // namespace

namespace i3d {

int track_sdf_chunks(const Model& m, const i3d_track_sdf_desc* d, const double* intr, const double* dist, const TrackSdfFrames& fr, double* poses6_io,
                     i3d_track_sdf_stats* stats, const TrackSdfRgbd* rgbd, int max_chunk, const TrackSdfDebug* debug) {
    hipStream_t st = m.stream; TrackSdfBuffers& buf = m.buf.track_sdf;
    const int32_t num = fr.num;
    TrackSdfPhoto ph{nullptr, 0.0, 0.0, 0.0};
    if (rgbd) {                                             // the intensity volume: once per call, from the fields as they stand now
        const double* vol = nullptr;
        if (rgbd->photo_weight > 0.0) if (int rc = m.fill_intensity(vol)) return rc;
        ph = photo_of(*rgbd, vol);
    }
    const int count_col = count_col_of(rgbd);
    const TrackSdfParams prm = make_params(d, intr, dist, fr.w, fr.h, m.row_cap);
    const int rows = register_rows(prm.n, prm.per_lane);
    const size_t px = (size_t)fr.w * fr.h;
    const size_t slab_bytes = (size_t)rows * TRACK_COLS * sizeof(double);
    const size_t frame_bytes = (fr.host_depth ? px * sizeof(float) : 0) + (fr.host_lum ? px * sizeof(float) : 0) + (rgbd ? 2 : 1) * sizeof(float*) +
                               3 * sizeof(double) + sizeof(TrackState) + slab_bytes;
    const int chunk = chunk_frames(frame_bytes, num, max_chunk);

    // the scratch of a chunk: depth copies | luminance copies | pointer table | luminance pointer table | pivots | states | slabs; every piece 256-byte aligned.
    // The tables, pivots and states are the head: one host image, uploaded in one copy
    size_t total = 0;
    auto take = [&total](size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_depth = take(fr.host_depth ? (size_t)chunk * px * sizeof(float) : 0), o_lum = take(fr.host_lum ? (size_t)chunk * px * sizeof(float) : 0);
    const size_t o_head = total, o_table = take((size_t)chunk * sizeof(float*)), o_ltable = take(rgbd ? (size_t)chunk * sizeof(float*) : 0),
                 o_pivot = take((size_t)chunk * 3 * sizeof(double));
    const size_t o_state = take((size_t)chunk * sizeof(TrackState)), head_bytes = total - o_head, o_slab = take((size_t)chunk * slab_bytes);
    MODEL_HIP(m, buf.scratch.alloc(total));
    unsigned char* base = buf.scratch.p;
    TrackState* d_state = (TrackState*)(base + o_state);
    TrackSdfBatch b{(const float* const*)(base + o_table), (const float* const*)(base + o_ltable), d_state, (const double*)(base + o_pivot), (double*)(base + o_slab), 0};

    // the pinned staging: the host image of the head | the states read back | the start poses | the usable counts.  The head is unchanged between an upload and
    // the next synchronisation, and every call ends on one
    size_t stage = 0;
    auto hold = [&stage](size_t bytes) { const size_t at = stage; stage += (bytes + 63) & ~(size_t)63; return at; };
    const size_t s_head = hold(head_bytes), s_back = hold((size_t)chunk * sizeof(TrackState)), s_start = hold((size_t)chunk * sizeof(Pose)),
                 s_usable = hold((size_t)chunk * sizeof(double));
    MODEL_HIP(m, buf.staging.alloc(stage));
    unsigned char* head = buf.staging.p + s_head;
    const float** h_table = (const float**)(head + (o_table - o_head));
    const float** h_ltable = (const float**)(head + (o_ltable - o_head));
    double* h_pivot = (double*)(head + (o_pivot - o_head));
    TrackState* h_state = (TrackState*)(head + (o_state - o_head));
    TrackState* back = (TrackState*)(buf.staging.p + s_back);
    Pose* start = (Pose*)(buf.staging.p + s_start);
    double* usable = (double*)(buf.staging.p + s_usable);
    const int budget = debug ? 0 : d->iterations;
    for (int f0 = 0; f0 < num; f0 += chunk) {
        const int nb = std::min(chunk, num - f0);
        b.frames = nb;
        if (fr.host_depth) MODEL_HIP(m, hipMemcpyAsync(base + o_depth, fr.host_depth + (size_t)f0 * px, (size_t)nb * px * sizeof(float), hipMemcpyHostToDevice, st));
        if (fr.host_lum) MODEL_HIP(m, hipMemcpyAsync(base + o_lum, fr.host_lum + (size_t)f0 * px, (size_t)nb * px * sizeof(float), hipMemcpyHostToDevice, st));
        std::memset(head, 0, head_bytes);
        for (int i = 0; i < nb; ++i) {                      // the pivot pass reads the start pose itself from the state
            h_table[i] = fr.host_depth ? (const float*)(base + o_depth) + (size_t)i * px : fr.dev_depth[f0 + i];
            if (rgbd) h_ltable[i] = fr.host_lum ? (const float*)(base + o_lum) + (size_t)i * px : fr.dev_lum[f0 + i];
            start[i] = pose_from_vec6(poses6_io + 6 * (size_t)(f0 + i));      // camera -> world: x = R p + t
            for (int k = 0; k < 9; ++k) h_state[i].R[k] = start[i].R[k];
            for (int a = 0; a < 3; ++a) h_state[i].t[a] = start[i].t[a];
            usable[i] = 0.0;
        }
        if (debug) {
            for (int a = 0; a < 3; ++a) h_pivot[a] = debug->pivot3[a];
        } else {                                            // the pivots: c = R0 mean(p) + t0 over the usable samples that count, fixed for the call
            MODEL_HIP(m, hipMemcpyAsync(base + o_head, head, head_bytes, hipMemcpyHostToDevice, st));
            launch_track_sdf_mean(st, prm, b, m.voxel_size);
            launch_track_solve(st, d_state, b.slab, nb, rows, 1, 28, 0.0, 0.0);
            MODEL_HIP(m, hipGetLastError());
            MODEL_HIP(m, hipMemcpyAsync(back, d_state, (size_t)nb * sizeof(TrackState), hipMemcpyDeviceToHost, st));
            MODEL_HIP(m, hipStreamSynchronize(st));
            for (int i = 0; i < nb; ++i) {
                pivot_of(back[i].sums, start[i].R, start[i].t, h_pivot + 3 * i);
                usable[i] = back[i].sums[TRACK_SDF_MEAN_COL_USABLE];      // does not depend on the pose: the pivot pass counts it for the rgbd form
            }
        }
        for (int i = 0; i < nb; ++i) start_state(h_state[i], start[i].R, start[i].t, h_pivot + 3 * i);
        MODEL_HIP(m, hipMemcpyAsync(base + o_head, head, head_bytes, hipMemcpyHostToDevice, st));
        for (int it = 0; it < budget; ++it) {               // back to back; a frame that is done costs nothing more, and once all are the launches are empty
            m.track_sdf_pass(prm, rgbd ? &ph : nullptr, b, 1);
            launch_track_solve(st, d_state, b.slab, nb, rows, 0, count_col, d->stop_rotation, d->stop_translation);
        }
        m.track_sdf_pass(prm, rgbd ? &ph : nullptr, b, 0);          // the figures at the returned poses: totals only
        launch_track_solve(st, d_state, b.slab, nb, rows, 1, 28, 0.0, 0.0);
        MODEL_HIP(m, hipGetLastError());
        MODEL_HIP(m, hipMemcpyAsync(back, d_state, (size_t)nb * sizeof(TrackState), hipMemcpyDeviceToHost, st));
        MODEL_HIP(m, hipStreamSynchronize(st));
        if (debug) {
            const double* sums = back[0].sums;
            for (int c = 0; c < TRACK_SUMS; ++c) debug->sums[c] = sums[c];
            if (debug->valid) *debug->valid = (int64_t)sums[TRACK_SUMS];
            if (debug->usable) *debug->usable = (int64_t)sums[TRACK_SDF_COL_USABLE];
            if (rgbd) {                                     // sums31: the photometric r^2 and sample count appended, as i3d_debug_track_rgbd_sums
                debug->sums[29] = sums[TRACK_COL_PHOTO_SQ]; debug->sums[30] = sums[TRACK_COL_PHOTO_N];
                if (debug->photo_samples) *debug->photo_samples = (int64_t)sums[TRACK_COL_PHOTO_N];
            }
            return I3D_OK;
        }
        for (int i = 0; i < nb; ++i)
            finish_frame(back[i], budget, h_pivot + 3 * i, poses6_io + 6 * (size_t)(f0 + i), stats ? stats + f0 + i : nullptr, rgbd, usable[i],
                         rgbd && rgbd->stats ? rgbd->stats + f0 + i : nullptr);
    }
    return I3D_OK;
}

int track_sdf_run(const Model& m, const i3d_track_sdf_desc* d, int32_t w, int32_t h, const float* depth, double* pose6_io, i3d_track_sdf_stats* stats,
                  const TrackSdfRgbd* rgbd, const float* luminance, const TrackSdfDebug* debug) {
    const std::string& fn = m.fn;
    if (!d) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    if (!depth) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null depth");
    if (rgbd && !luminance) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null luminance");
    if (!pose6_io) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null pose");
    if (int rc = check_desc(m, d, w, h)) return rc;
    if (rgbd) if (int rc = check_rgbd(m, *rgbd)) return rc;
    if (int rc = m.check_pose(pose6_io)) return rc;
    const double* intr = d->intrinsics4; const double* dist = d->distortion5;
    if (int rc = m.ready(d->use_context_camera != 0, intr, dist)) return rc;
    if (!d->use_context_camera) if (int rc = m.check_focal(intr)) return rc;
    if (rgbd && rgbd->photo_weight > 0.0) if (int rc = m.intensity_ready()) return rc;
    return track_sdf_chunks(m, d, intr, dist, TrackSdfFrames{1, w, h, depth, nullptr, luminance, nullptr}, pose6_io, stats, rgbd, 0, debug);
}

}  // namespace i3d

namespace {

// ---- a batch of frames ----------------------------------------------------------------------------------------------------------------
// the driver for the two batch entry points after their checks, on the context's device
int context_chunks(const ContextModel& m, const i3d_track_sdf_desc* d, const double* intr, const double* dist, const TrackSdfFrames& fr, double* poses6_io,
                   i3d_track_sdf_stats* stats, const TrackSdfRgbd* rgbd) {
    if (int rc = m.make_current()) return rc;
    return track_sdf_chunks(m, d, intr, dist, fr, poses6_io, stats, rgbd, m.c->track_batch_frames);
}

// the checks the two batch entry points share, in the order of track_sdf_run: the size and the descriptor, the start poses
int batch_checks(const Model& m, const i3d_track_sdf_desc* d, int32_t num, int32_t w, int32_t h, const double* poses6) {
    if (int rc = check_desc(m, d, w, h)) return rc;
    for (int32_t f = 0; f < num; ++f)
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(poses6[6 * (size_t)f + k])) return m.fail(I3D_ERR_INVALID_ARGUMENT, m.fn + ": the pose of frame " + std::to_string(f) + " is not finite");
    return I3D_OK;
}

// the photometric checks of a batch call, after batch_checks: the descriptor's, then the state's
int batch_rgbd_checks(const Model& m, const TrackSdfRgbd* rgbd) {
    if (!rgbd) return I3D_OK;
    if (int rc = check_rgbd(m, *rgbd)) return rc;
    return rgbd->photo_weight > 0.0 ? m.intensity_ready() : I3D_OK;
}

// i3d_track_frames_sdf, and with rgbd i3d_track_frames_sdf_rgbd
int track_frames_entry(i3d_context* c, const std::string& fn, const i3d_track_sdf_desc* d, int32_t num, int32_t w, int32_t h, const float* depth, const float* lum,
                       double* poses6_io, i3d_track_sdf_stats* stats, const TrackSdfRgbd* rgbd) {
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null context");
    if (!d) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    if (num < 0) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": num_frames must be >= 0");
    if (num == 0) return I3D_OK;
    if (!depth) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null depth");
    if (rgbd && !lum) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null luminance");
    if (!poses6_io) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null poses");
    const ContextModel m(c, fn, d->use_refined_sdf != 0);
    if (int rc = batch_checks(m, d, num, w, h, poses6_io)) return rc;
    const double* intr = d->intrinsics4; const double* dist = d->distortion5;
    if (int rc = m.check_state(d->use_context_camera != 0, intr, dist)) return rc;
    if (!d->use_context_camera) if (int rc = m.check_focal(intr)) return rc;
    if (int rc = batch_rgbd_checks(m, rgbd)) return rc;
    return context_chunks(m, d, intr, dist, TrackSdfFrames{num, w, h, depth, nullptr, lum, nullptr}, poses6_io, stats, rgbd);
}

// i3d_track_keyframes_sdf, and with rgbd i3d_track_keyframes_sdf_rgbd: both pointer tables at the resident images of the level
int track_keyframes_entry(i3d_context* c, const std::string& fn, const i3d_track_sdf_desc* d, int32_t level, int32_t num, const int32_t* frames, double* poses6_io,
                          i3d_track_sdf_stats* stats, const TrackSdfRgbd* rgbd) {
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null context");
    if (!d) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    if (num < 0) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": num must be >= 0");
    if (num == 0) return I3D_OK;
    if (!poses6_io) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null poses");
    if (!d->use_context_camera) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": desc->use_context_camera must be 1 (the keyframes are the context camera's)");
    const ContextModel m(c, fn, d->use_refined_sdf != 0);
    if (int rc = m.check_field()) return rc;
    if (!c->have_frames) return ctx_fail(c, I3D_ERR_STATE, fn + ": no keyframes (i3d_set_frames)");
    if (!c->have_camera) return ctx_fail(c, I3D_ERR_STATE, fn + ": no camera (i3d_set_camera)");
    if (level < 0 || level >= c->levels) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": level out of range");
    if (!frames && num != c->K) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": without frame indices num must be the number of keyframes");
    std::vector<const float*> images(num), lums(num);
    for (int32_t i = 0; i < num; ++i) {
        const int32_t f = frames ? frames[i] : i;
        if (f < 0 || f >= c->K) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": keyframe index " + std::to_string(f) + " out of range");
        images[i] = c->depth[(size_t)f * c->levels + level].p;
        lums[i] = c->lum[(size_t)f * c->levels + level].p;
    }
    const int32_t w = c->fw[level], h = c->fh[level];
    if (int rc = batch_checks(m, d, num, w, h, poses6_io)) return rc;
    if (int rc = batch_rgbd_checks(m, rgbd)) return rc;
    double intr[4];
    for (int i = 0; i < 4; ++i) intr[i] = std::ldexp(c->intr[i], -level);      // all four x 2^-level, exact (section 13.1 item 1)
    return context_chunks(m, d, intr, c->dist, TrackSdfFrames{num, w, h, nullptr, images.data(), nullptr, lums.data()}, poses6_io, stats, rgbd);
}

}  // namespace

extern "C" int i3d_track_frames_sdf(i3d_context* c, const i3d_track_sdf_desc* d, int32_t num, int32_t w, int32_t h, const float* depth, double* poses6_io,
                                    i3d_track_sdf_stats* stats) {
    return track_frames_entry(c, "i3d_track_frames_sdf", d, num, w, h, depth, nullptr, poses6_io, stats, nullptr);
}

extern "C" int i3d_track_keyframes_sdf(i3d_context* c, const i3d_track_sdf_desc* d, int32_t level, int32_t num, const int32_t* frames, double* poses6_io,
                                       i3d_track_sdf_stats* stats) {
    return track_keyframes_entry(c, "i3d_track_keyframes_sdf", d, level, num, frames, poses6_io, stats, nullptr);
}

extern "C" int i3d_debug_track_batch_frames(i3d_context* c, int32_t frames_per_chunk) {
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_debug_track_batch_frames: null context");
    c->track_batch_frames = frames_per_chunk > 0 ? frames_per_chunk : 0;
    return I3D_OK;
}

extern "C" void i3d_track_sdf_desc_default(i3d_track_sdf_desc* d) {
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    d->use_refined_sdf = 1; d->iterations = 30; d->stride = 1; d->max_distance = 0.05; d->stop_rotation = 1e-6; d->stop_translation = 1e-6;
}

extern "C" int i3d_track_frame_sdf(i3d_context* c, const i3d_track_sdf_desc* d, int32_t w, int32_t h, const float* depth, double* pose6_io,
                                   i3d_track_sdf_stats* stats) {
    const char* fn = "i3d_track_frame_sdf";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null context");
    return track_sdf_run(ContextModel(c, fn, d && d->use_refined_sdf != 0), d, w, h, depth, pose6_io, stats);
}

extern "C" int i3d_debug_track_sdf_sums(i3d_context* c, const i3d_track_sdf_desc* d, int32_t w, int32_t h, const float* depth, const double* pose6,
                                        const double* pivot3, double* sums29, int64_t* valid, int64_t* valid_pixels) {
    const char* fn = "i3d_debug_track_sdf_sums";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null context");
    if (!pose6 || !pivot3 || !sums29) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null argument");
    double pose[6];
    for (int k = 0; k < 6; ++k) pose[k] = pose6[k];
    const TrackSdfDebug dbg{pivot3, sums29, valid, valid_pixels, nullptr};
    return track_sdf_run(ContextModel(c, fn, d && d->use_refined_sdf != 0), d, w, h, depth, pose, nullptr, nullptr, nullptr, &dbg);
}

// ---- the photometric term on the field ------------------------------------------------------------------------------------------------
extern "C" void i3d_track_sdf_rgbd_desc_default(i3d_track_sdf_rgbd_desc* d) {
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    i3d_track_sdf_desc_default(&d->base);
    d->geometric_weight = 1.0;
    d->photo_weight = 0.1;                       // metres per unit luminance, as i3d_track_rgbd_desc
    d->max_photo_residual = 0.0f;                // open
}

extern "C" int i3d_track_frame_sdf_rgbd(i3d_context* c, const i3d_track_sdf_rgbd_desc* d, int32_t w, int32_t h, const float* depth, const float* luminance,
                                        double* pose6_io, i3d_track_sdf_rgbd_stats* stats) {
    const char* fn = "i3d_track_frame_sdf_rgbd";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null context");
    if (!d) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null descriptor");
    const TrackSdfRgbd r = rgbd_of(d, stats);
    return track_sdf_run(ContextModel(c, fn, d->base.use_refined_sdf != 0), &d->base, w, h, depth, pose6_io, nullptr, &r, luminance);
}

extern "C" int i3d_track_frames_sdf_rgbd(i3d_context* c, const i3d_track_sdf_rgbd_desc* d, int32_t num, int32_t w, int32_t h, const float* depth,
                                         const float* luminance, double* poses6_io, i3d_track_sdf_rgbd_stats* stats) {
    const std::string fn = "i3d_track_frames_sdf_rgbd";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null context");
    if (!d) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    const TrackSdfRgbd r = rgbd_of(d, stats);
    return track_frames_entry(c, fn, &d->base, num, w, h, depth, luminance, poses6_io, nullptr, &r);
}

extern "C" int i3d_track_keyframes_sdf_rgbd(i3d_context* c, const i3d_track_sdf_rgbd_desc* d, int32_t level, int32_t num, const int32_t* frames,
                                            double* poses6_io, i3d_track_sdf_rgbd_stats* stats) {
    const std::string fn = "i3d_track_keyframes_sdf_rgbd";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null context");
    if (!d) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    const TrackSdfRgbd r = rgbd_of(d, stats);
    return track_keyframes_entry(c, fn, &d->base, level, num, frames, poses6_io, nullptr, &r);
}

extern "C" int i3d_debug_track_sdf_rgbd_sums(i3d_context* c, const i3d_track_sdf_rgbd_desc* d, int32_t w, int32_t h, const float* depth, const float* luminance,
                                             const double* pose6, const double* pivot3, double* sums31, int64_t* valid, int64_t* photo_samples) {
    const char* fn = "i3d_debug_track_sdf_rgbd_sums";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null context");
    if (!d || !pose6 || !pivot3 || !sums31) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null argument");
    double pose[6];
    for (int k = 0; k < 6; ++k) pose[k] = pose6[k];
    const TrackSdfRgbd r = rgbd_of(d, nullptr);
    const TrackSdfDebug dbg{pivot3, sums31, valid, nullptr, photo_samples};
    return track_sdf_run(ContextModel(c, fn, d->base.use_refined_sdf != 0), &d->base, w, h, depth, pose, nullptr, &r, luminance, &dbg);
}

extern "C" int i3d_debug_voxel_intensity(i3d_context* c, int32_t use_refined_sdf, double* out) {
    const std::string fn = "i3d_debug_voxel_intensity";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null context");
    if (!out) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null output");
    const ContextModel m(c, fn, use_refined_sdf != 0);
    if (int rc = m.check_field()) return rc;
    if (int rc = m.intensity_ready()) return rc;
    if (int rc = m.make_current()) return rc;
    const double* vol = nullptr;
    if (int rc = m.fill_intensity(vol)) return rc;
    DevBuf<double> visit;
    CTX_HIP(c, visit.alloc((size_t)c->N));
    launch_gather_visit(c->stream, c->N, c->rank.p, vol, nullptr, visit.p, nullptr);
    CTX_HIP(c, hipGetLastError());
    CTX_HIP(c, hipMemcpyAsync(out, visit.p, sizeof(double) * (size_t)c->N, hipMemcpyDeviceToHost, c->stream));
    CTX_HIP(c, hipStreamSynchronize(c->stream));
    return I3D_OK;
}
