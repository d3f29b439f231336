// i3d_track_frame_sdf: registration of a depth frame on the stored field, no ray cast (track_sdf_kernels.hip; the definition is DESIGN.md section 19).
// track_sdf_run is the driver for every model (the context here, the fusion volume in fusion.cpp): validation, the camera, one grown-only scratch, one upload of
// the depth, the pivot, the whole budget launched back to back, the figures at the returned pose; two stream synchronisations.  The pose comes in and goes out
// world -> camera, as i3d_track_frame's; the loop runs on its inverse, the camera -> world pose of section 18.  Reads the grid and, with use_context_camera, the
// context's camera; writes only its scratch, nothing any other entry point reads.
// i3d_track_frames_sdf / i3d_track_keyframes_sdf: track_sdf_batch_run runs the same loop for a chunk of frames at once - the batch
// kernels, k_track_solve with one workgroup per frame - with two synchronisations per chunk; validation, parameters, pivot, start state and figures are the
// single-frame driver's own functions.
#include <algorithm>
#include "context.hpp"

using namespace i3d;

namespace {

constexpr int TRACK_SDF_MAX_EDGE = 1 << 15;
constexpr int TRACK_SDF_MAX_STRIDE = 16;
constexpr int TRACK_SDF_MAX_ITERATIONS = 200;

#define S_HIP(m, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (m).fail(I3D_ERR_HIP, std::string(#expr) + " -> " + hipGetErrorString(e_)); } while (0)

double rms_of(double sq, double n) { return n > 0.0 ? std::sqrt(sq / n) : 0.0; }

using Fail = std::function<int(int code, const std::string& msg)>;

// the size and descriptor faults of section 19, one text for the single frame and the batch
int check_desc(const Fail& fail, const std::string& fn, const i3d_track_sdf_desc* d, int32_t w, int32_t h) {
    if (w <= 0 || h <= 0 || w > TRACK_SDF_MAX_EDGE || h > TRACK_SDF_MAX_EDGE) return fail(I3D_ERR_INVALID_ARGUMENT, fn + ": image size out of range");
    if (d->stride < 1 || d->stride > TRACK_SDF_MAX_STRIDE) return fail(I3D_ERR_INVALID_ARGUMENT, fn + ": stride must be 1.." + std::to_string(TRACK_SDF_MAX_STRIDE));
    if (d->iterations < 0 || d->iterations > TRACK_SDF_MAX_ITERATIONS)
        return fail(I3D_ERR_INVALID_ARGUMENT, fn + ": iterations must be 0.." + std::to_string(TRACK_SDF_MAX_ITERATIONS));
    if (!std::isfinite(d->max_distance) || !(d->max_distance > 0.0)) return fail(I3D_ERR_INVALID_ARGUMENT, fn + ": max_distance must be finite and > 0");
    if (!std::isfinite(d->huber_delta)) return fail(I3D_ERR_INVALID_ARGUMENT, fn + ": huber_delta must be finite (<= 0: off)");
    return I3D_OK;
}

// the kernels' parameters of a frame of w x h under the camera intr / dist; the pivot is left 0
TrackSdfParams make_params(const i3d_track_sdf_desc* d, const double* intr, const double* dist, int32_t w, int32_t h, int row_cap) {
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
    prm.per_lane = register_per_lane(n, row_cap);
    return prm;
}

// the pivot c = R0 mean(p) + t0 from the totals of the mean pass (columns 0..2 the sum, 3 the number)
void pivot_of(const double* sums, const double* R0, const double* t0, double* c) {
    double mean[3] = {0.0, 0.0, 0.0};
    if (sums[3] > 0.0) for (int a = 0; a < 3; ++a) mean[a] = sums[a] / sums[3];
    for (int a = 0; a < 3; ++a) c[a] = ((R0[3 * a] * mean[0] + R0[3 * a + 1] * mean[1]) + R0[3 * a + 2] * mean[2]) + t0[a];
}

// the state a loop starts from: the start pose about the pivot
void start_state(TrackState& hs, const double* R0, const double* t0, const double* c) {
    std::memset(&hs, 0, sizeof(hs));
    for (int i = 0; i < 9; ++i) hs.R[i] = R0[i];
    for (int a = 0; a < 3; ++a) hs.t[a] = t0[a] - c[a];
    hs.status = 1; hs.first = 1;
}

// the figures of section 19.1 from the state after the figures pass, and the pose when a step was applied
void finish_frame(const TrackState& hs, int budget, const double* c, double* pose6_io, i3d_track_sdf_stats* stats) {
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
        for (int a = 0; a < 3; ++a) Pn.t[a] = hs.t[a] + c[a];
        vec6_from_pose(Pn, pose6_io);
    }
    if (stats) *stats = out;
}

}  // namespace

namespace i3d {

int track_sdf_run(hipStream_t st, DevBuf<unsigned char>& scratch, const TrackSdfModel& m, const char* what, const i3d_track_sdf_desc* d, int32_t w, int32_t h,
                  const float* depth, double* pose6_io, i3d_track_sdf_stats* stats, const double* debug_pivot3, double* debug_sums29, int64_t* debug_valid,
                  int64_t* debug_usable) {
    const std::string fn(what);
    if (!d) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    if (!depth) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null depth");
    if (!pose6_io) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null pose");
    if (int rc = check_desc(m.fail, fn, d, w, h)) return rc;
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(pose6_io[k])) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": the pose is not finite");
    const double* intr = d->intrinsics4; const double* dist = d->distortion5;
    if (int rc = m.ready(*d, intr, dist)) return rc;
    if (!d->use_context_camera && (!(intr[0] > 0.0) || !(intr[1] > 0.0))) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": focal lengths must be > 0");

    TrackSdfParams prm = make_params(d, intr, dist, w, h, m.row_cap);

    // the scratch: depth | slab | state; every piece 256-byte aligned
    const int rows = register_rows(prm.n, prm.per_lane);
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
        pivot_of(hs.sums, R0, t0, prm.c);
    }
    start_state(hs, R0, t0, prm.c);
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
    finish_frame(hs, budget, prm.c, pose6_io, stats);
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

// ---- a batch of frames ----------------------------------------------------------------------------------------------------------------
constexpr size_t TRACK_SDF_BATCH_BYTES = (size_t)512 << 20;     // the scratch of a chunk at most (a single frame may exceed it: a chunk holds at least one)
constexpr int TRACK_SDF_BATCH_MAX = 65535;                      // frames of a chunk at most: gridDim.y

// frames per chunk (section 20.3): the largest number whose scratch stays within TRACK_SDF_BATCH_BYTES, at least 1, at most TRACK_SDF_BATCH_MAX; the debug value
// of the context lowers it
int chunk_frames(const i3d_context* c, size_t frame_bytes, int num) {
    long long n = (long long)(TRACK_SDF_BATCH_BYTES / frame_bytes);
    n = std::max(1LL, std::min(n, (long long)TRACK_SDF_BATCH_MAX));
    if (c->track_batch_frames > 0) n = std::min(n, (long long)c->track_batch_frames);
    return (int)std::min(n, (long long)num);
}

// The driver of i3d_track_frames_sdf / i3d_track_keyframes_sdf after their own checks: `num` frames of w x h under the camera intr / dist.  host_depth: the
// frames' images [num][h][w], uploaded chunk by chunk; null: dev_depth[num] are resident device images and nothing is uploaded.  Per chunk: the upload, the
// batched pivot pass and solve, one synchronisation, the pivots and start states formed on the host, the whole budget launched back to back, the figures pass,
// one read-back and a second synchronisation.  A frame's launches, sums and host arithmetic are those of track_sdf_run, so its result has that call's bits.
int track_sdf_batch_run(i3d_context* c, const std::string& fn, const i3d_track_sdf_desc* d, const double* intr, const double* dist, int32_t num, int32_t w, int32_t h,
                        const float* host_depth, const float* const* dev_depth, double* poses6_io, i3d_track_sdf_stats* stats) {
    CTX_HIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const TrackSdfParams prm = make_params(d, intr, dist, w, h, c->register_row_cap);
    const int rows = register_rows(prm.n, prm.per_lane);
    const size_t px = (size_t)w * h;
    const size_t slab_bytes = (size_t)rows * TRACK_COLS * sizeof(double);
    const size_t frame_bytes = (host_depth ? px * sizeof(float) : 0) + sizeof(float*) + 3 * sizeof(double) + sizeof(TrackState) + slab_bytes;
    const int chunk = chunk_frames(c, frame_bytes, num);

    // the scratch of a chunk: depth copies | pointer table | pivots | states | slabs; every piece 256-byte aligned.  table | pivots | states is the head: one
    // host image, uploaded in one copy
    size_t total = 0;
    auto take = [&total](size_t bytes) { const size_t at = total; total += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_depth = take(host_depth ? (size_t)chunk * px * sizeof(float) : 0);
    const size_t o_head = total, o_table = take((size_t)chunk * sizeof(float*)), o_pivot = take((size_t)chunk * 3 * sizeof(double));
    const size_t o_state = take((size_t)chunk * sizeof(TrackState)), head_bytes = total - o_head, o_slab = take((size_t)chunk * slab_bytes);
    CTX_HIP(c, c->track_sdf_batch_scratch.alloc(total));
    unsigned char* base = c->track_sdf_batch_scratch.p;
    TrackState* d_state = (TrackState*)(base + o_state);
    TrackSdfBatch b{(const float* const*)(base + o_table), d_state, (const double*)(base + o_pivot), (double*)(base + o_slab), 0};
    const bool refined = d->use_refined_sdf != 0;
    const RenderGrid g{HashTable{c->hkeys.p, c->hvals.p, c->hmask}, c->nbr.p, c->N, c->weight.p, refined ? c->x_sdf.p : c->sdf0.p, c->x_alb.p, c->sh.p,
                       (double)c->voxel_size, nullptr, {0, 0, 0}, {0, 0, 0}};

    std::vector<unsigned char> head(head_bytes);            // the host image of the head; unchanged between an upload and the next synchronisation
    const float** h_table = (const float**)(head.data() + (o_table - o_head));
    double* h_pivot = (double*)(head.data() + (o_pivot - o_head));
    TrackState* h_state = (TrackState*)(head.data() + (o_state - o_head));
    std::vector<TrackState> back(chunk);
    std::vector<Pose> start(chunk);
    const int budget = d->iterations;
    for (int f0 = 0; f0 < num; f0 += chunk) {
        const int nb = std::min(chunk, num - f0);
        b.frames = nb;
        if (host_depth) CTX_HIP(c, hipMemcpyAsync(base + o_depth, host_depth + (size_t)f0 * px, (size_t)nb * px * sizeof(float), hipMemcpyHostToDevice, st));
        std::memset(head.data(), 0, head_bytes);
        for (int i = 0; i < nb; ++i) {                      // the pivot pass reads the start pose itself from the state
            h_table[i] = host_depth ? (const float*)(base + o_depth) + (size_t)i * px : dev_depth[f0 + i];
            start[i] = pose_from_vec6(poses6_io + 6 * (size_t)(f0 + i));      // camera -> world: x = R p + t
            for (int k = 0; k < 9; ++k) h_state[i].R[k] = start[i].R[k];
            for (int a = 0; a < 3; ++a) h_state[i].t[a] = start[i].t[a];
        }
        CTX_HIP(c, hipMemcpyAsync(base + o_head, head.data(), head_bytes, hipMemcpyHostToDevice, st));
        launch_track_sdf_mean_batch(st, prm, b, (double)c->voxel_size);
        launch_track_solve_batch(st, d_state, b.slab, nb, rows, 1, 28, 0.0, 0.0);
        CTX_HIP(c, hipGetLastError());
        CTX_HIP(c, hipMemcpyAsync(back.data(), d_state, (size_t)nb * sizeof(TrackState), hipMemcpyDeviceToHost, st));
        CTX_HIP(c, hipStreamSynchronize(st));
        for (int i = 0; i < nb; ++i) {
            pivot_of(back[i].sums, start[i].R, start[i].t, h_pivot + 3 * i);
            start_state(h_state[i], start[i].R, start[i].t, h_pivot + 3 * i);
        }
        CTX_HIP(c, hipMemcpyAsync(base + o_head, head.data(), head_bytes, hipMemcpyHostToDevice, st));
        for (int it = 0; it < budget; ++it) {               // back to back; a frame that is done costs nothing more, and once all are the launches are empty
            launch_track_sdf_batch(st, g, prm, b, 1);
            launch_track_solve_batch(st, d_state, b.slab, nb, rows, 0, 28, d->stop_rotation, d->stop_translation);
        }
        launch_track_sdf_batch(st, g, prm, b, 0);           // the figures at the returned poses: totals only
        launch_track_solve_batch(st, d_state, b.slab, nb, rows, 1, 28, 0.0, 0.0);
        CTX_HIP(c, hipGetLastError());
        CTX_HIP(c, hipMemcpyAsync(back.data(), d_state, (size_t)nb * sizeof(TrackState), hipMemcpyDeviceToHost, st));
        CTX_HIP(c, hipStreamSynchronize(st));
        for (int i = 0; i < nb; ++i) finish_frame(back[i], budget, h_pivot + 3 * i, poses6_io + 6 * (size_t)(f0 + i), stats ? stats + f0 + i : nullptr);
    }
    return I3D_OK;
}

// the checks the two batch entry points share, in the order of track_sdf_run: null pointers, the count, the size and the descriptor, the start poses
int batch_checks(i3d_context* c, const std::string& fn, const i3d_track_sdf_desc* d, int32_t num, int32_t w, int32_t h, const double* poses6) {
    const Fail fail = [c](int code, const std::string& msg) { return ctx_fail(c, code, msg); };
    if (int rc = check_desc(fail, fn, d, w, h)) return rc;
    for (int32_t f = 0; f < num; ++f)
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(poses6[6 * (size_t)f + k])) return fail(I3D_ERR_INVALID_ARGUMENT, fn + ": the pose of frame " + std::to_string(f) + " is not finite");
    return I3D_OK;
}

}  // namespace

extern "C" int i3d_track_frames_sdf(i3d_context* c, const i3d_track_sdf_desc* d, int32_t num, int32_t w, int32_t h, const float* depth, double* poses6_io,
                                    i3d_track_sdf_stats* stats) {
    const std::string fn = "i3d_track_frames_sdf";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null context");
    if (!d) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    if (num < 0) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": num_frames must be >= 0");
    if (num == 0) return I3D_OK;
    if (!depth) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null depth");
    if (!poses6_io) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null poses");
    if (int rc = batch_checks(c, fn, d, num, w, h, poses6_io)) return rc;
    const double* intr = d->intrinsics4; const double* dist = d->distortion5;
    if (!c->have_grid) return ctx_fail(c, I3D_ERR_STATE, fn + ": no grid");
    if (d->use_context_camera) {
        if (!c->have_camera) return ctx_fail(c, I3D_ERR_STATE, fn + ": use_context_camera without a camera (i3d_set_camera)");
        intr = c->intr; dist = c->dist;
    } else if (!(intr[0] > 0.0) || !(intr[1] > 0.0)) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": focal lengths must be > 0");
    return track_sdf_batch_run(c, fn, d, intr, dist, num, w, h, depth, nullptr, poses6_io, stats);
}

extern "C" int i3d_track_keyframes_sdf(i3d_context* c, const i3d_track_sdf_desc* d, int32_t level, int32_t num, const int32_t* frames, double* poses6_io,
                                       i3d_track_sdf_stats* stats) {
    const std::string fn = "i3d_track_keyframes_sdf";
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null context");
    if (!d) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    if (num < 0) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": num must be >= 0");
    if (num == 0) return I3D_OK;
    if (!poses6_io) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": null poses");
    if (!d->use_context_camera) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": desc->use_context_camera must be 1 (the keyframes are the context camera's)");
    if (!c->have_grid) return ctx_fail(c, I3D_ERR_STATE, fn + ": no grid");
    if (!c->have_frames) return ctx_fail(c, I3D_ERR_STATE, fn + ": no keyframes (i3d_set_frames)");
    if (!c->have_camera) return ctx_fail(c, I3D_ERR_STATE, fn + ": no camera (i3d_set_camera)");
    if (level < 0 || level >= c->levels) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": level out of range");
    if (!frames && num != c->K) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": without frame indices num must be the number of keyframes");
    std::vector<const float*> images(num);
    for (int32_t i = 0; i < num; ++i) {
        const int32_t f = frames ? frames[i] : i;
        if (f < 0 || f >= c->K) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, fn + ": keyframe index " + std::to_string(f) + " out of range");
        images[i] = c->depth[(size_t)f * c->levels + level].p;
    }
    const int32_t w = c->fw[level], h = c->fh[level];
    if (int rc = batch_checks(c, fn, d, num, w, h, poses6_io)) return rc;
    double intr[4];
    for (int i = 0; i < 4; ++i) intr[i] = std::ldexp(c->intr[i], -level);      // all four x 2^-level, exact (section 13.1 item 1)
    return track_sdf_batch_run(c, fn, d, intr, c->dist, num, w, h, nullptr, images.data(), poses6_io, stats);
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
