// The model view: what a driver that reads the stored field - the ray cast, the trackers, the point query, the point-set registration,
// the depth frames on the field - may ask of a context or a fusion volume, stated once.  A handle holds one ModelBuffers by value and has one adapter
// (ContextModel in context.hpp, FusionModel in fusion_internal.hpp); the drivers below are written against Model alone and serve both.
#pragma once
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include "../device/render_kernels.hpp"
#include "../device/track_kernels.hpp"
#include "../device/query_kernels.hpp"
#include "../device/register_kernels.hpp"
#include "../device/track_sdf_kernels.hpp"
#include "../device/cast_rays_kernels.hpp"
#include "devbuf.hpp"
#include "../../../include/intrinsic3d_hip.h"

namespace i3d {

inline double rms_of(double sq, double n) { return n > 0.0 ? std::sqrt(sq / n) : 0.0; }

// frame registration (track.cpp): frame depth pyramid, frame vertex / normal planes, the model planes of a level's ray cast, the frame luminance pyramid
// (i3d_track_frame_rgbd only), the per-workgroup sums, the Gauss-Newton state
struct TrackBuffers {
    DevBuf<float> pyr, vn, model, lum; DevBuf<double> slab; DevBuf<TrackState> state; DevBuf<RenderStatsDev> rstats;
};
// depth frames on the field (track_sdf.cpp): the device scratch of a chunk and the pinned host image of its head with the states read back, the start poses and
// the usable counts
struct TrackSdfBuffers { DevBuf<unsigned char> scratch; PinnedBuf staging; };

// What the drivers keep between calls, one set per handle, grown only, read by nothing else
struct ModelBuffers {
    // the brick bitmap of the voxels with weight != 0 (ensure_bricks): cached until the handle changes its stored voxels and sets ok = false
    struct Bricks { DevBuf<unsigned> bits; DevBuf<int> bounds; int lo[3] = {0, 0, 0}, dim[3] = {0, 0, 0}; bool ok = false; } bricks;
    DevBuf<float> planes; DevBuf<RenderStatsDev> stats;            // render_run: the requested planes and the stats
    TrackBuffers track;
    DevBuf<unsigned char> query_scratch, register_scratch;         // query_run, register_run: the one scratch of a call
    DevBuf<unsigned char> cast_scratch;                            // cast_rays_run: the one scratch of a call
    TrackSdfBuffers track_sdf;
    // the fp64 intensity volume of the photometric term on the field, indexed as the corners of the grid's cell (the context: the voxel, the
    // fusion volume: the table slot); filled anew by every call that has a photometric weight and read by that call alone
    DevBuf<double> intensity;
};

struct Model {
    ModelBuffers& buf;
    int device; hipStream_t stream;
    double voxel_size;
    int row_cap;                    // slab rows of a pass at most (REGISTER_MAX_ROWS; lowered by i3d_debug_register_row_cap only)
    const char* noun;               // "grid" / "volume", for the messages
    const char* bitmap_owner;       // who the capacity message of the bitmap names ("i3d_render_view" / "fusion": it never named the caller)
    bool cast_intensity;            // the ray cast can write an intensity plane at all (the fusion volume's cannot: its colour is used on the field instead)
    std::string fn;                 // the entry point, for the messages

    virtual int fail(int code, const std::string& msg) const = 0;         // records the message with the handle, returns code
    // the model's own state checks, made after the descriptor's.  The context: a grid is resident; with use_context_camera a camera is, and intr / dist become
    // the context's.  The fusion volume: nothing (its entry points refuse use_context_camera themselves)
    virtual int check_state(bool use_context_camera, const double*& intr, const double*& dist) const = 0;
    virtual int intensity_ready() const = 0;                              // whether an intensity can be formed (the context: the per-voxel SH is there), else the error
    virtual size_t intensity_entries() const = 0;
    virtual void launch_intensity(double* vol) const = 0;
    // the launches that differ by grid type, on the model's stream
    virtual void brick_bounds(int* bounds) const = 0;
    virtual void brick_fill(unsigned* bits, const int lo[3], const int dim[3]) const = 0;
    virtual void cast(const RenderCam& cam, const RenderPlanes& out, RenderStatsDev* stats) const = 0;
    virtual void cast_rays(const CastRays& p, RenderStatsDev* stats) const = 0;      // the caller's own rays, over the cached bitmap as cast
    // the colour instantiations of the two: depth / t, status, the stored colour at the hit and the stats
    virtual void cast_color(const RenderCam& cam, const RenderColorPlanes& out, RenderStatsDev* stats) const = 0;
    virtual void cast_rays_color(const CastRaysColor& p, RenderStatsDev* stats) const = 0;
    virtual void query(const QueryParams& p, const double* points, const QueryOut& out, QueryRow* rows, QueryRow* total) const = 0;
    virtual void register_pass(const RegisterParams& p, const double* points, const TrackState* state, int check_done, double* slab) const = 0;
    virtual void track_sdf_pass(const TrackSdfParams& p, const TrackSdfPhoto* ph, const TrackSdfBatch& b, int check_done) const = 0;   // ph null: depth only

    int fail_hip(const char* what, hipError_t e) const { return fail(I3D_ERR_HIP, std::string(what) + " -> " + hipGetErrorString(e)); }
    int check_field() const { const double* none = nullptr; return check_state(false, none, none); }      // the state alone: no camera is asked for
    int make_current() const;                                             // hipSetDevice(device)
    int ready(bool use_context_camera, const double*& intr, const double*& dist) const {      // check_state, then the device made current
        if (int rc = check_state(use_context_camera, intr, dist)) return rc;
        return make_current();
    }
    int ready() const { const double* none = nullptr; return ready(false, none, none); }
    int fill_intensity(const double*& vol) const;                         // the intensity volume of the fields as they stand; no cache across calls
    // the descriptor checks more than one driver makes
    int check_focal(const double* intr) const;
    int check_pose(const double* pose6) const;
    int check_weights(double geometric, double photo) const;

protected:
    Model(ModelBuffers& b, int dev, hipStream_t st, double vs, int cap, const char* noun_, const char* owner, bool cast_int, const std::string& fn_)
        : buf(b), device(dev), stream(st), voxel_size(vs), row_cap(cap), noun(noun_), bitmap_owner(owner), cast_intensity(cast_int), fn(fn_) {}
    ~Model() = default;
};

// on a HIP error, record it with the model's handle and return I3D_ERR_HIP
#define MODEL_HIP(m, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (m).fail_hip(#expr, e_); } while (0)

// the cached brick bitmap of the model: bounds of the bricks that hold a voxel with weight != 0, then one bit per brick of that box; built on first use after the
// handle dropped it.  One stream synchronisation when it builds
int ensure_bricks(const Model& m);

// the pose part of a view's camera: distortion (zero below 1e-5), world -> camera rotation and centre of pose6, the camera-z clip (<= 0: open)
RenderCam render_cam(const PinholeCam& k, const double* pose6, float min_depth, float max_depth);
// the host images a ray cast is asked for (null: not requested).  colour_view: the colour view of DESIGN.md 35 (Model::cast_color), which has depth and
// color [h][w][3] alone; otherwise color is not read
struct RenderWant { float* depth; float* normal; float* albedo; float* shading; float* intensity; float* residual; float* color; bool colour_view; };
// after the entry point's checks and its choice of camera: the device made current, the bitmap, the plane scratch sized by the planes requested, one launch,
// the planes copied back, one synchronisation, the stats.  keyframe_lum: the device luminance a residual is taken against
int render_run(const Model& m, const RenderCam& cam, const RenderWant& want, const float* keyframe_lum, i3d_render_stats* stats);

// the photometric term of i3d_track_frame_rgbd: inputs, and the figures it adds to i3d_track_stats
struct TrackRgbd {
    const float* luminance; double geometric_weight, photo_weight; float max_photo_residual;
    int64_t photo_samples = 0; double photo_rms_initial = 0.0, photo_rms_final = 0.0;
};
// the loop of levels and passes, the stop rule, the status codes and the final figures of DESIGN.md 14.1: one definition for every model.  rgbd: null for the
// depth-only registration (k_track_assoc<false>), else the photometric term (k_track_assoc<true>)
int track_frame_run(const Model& m, const i3d_track_desc* d, int32_t w, int32_t h, const float* depth, double* pose6_io, i3d_track_stats* stats, TrackRgbd* rgbd = nullptr);
// one association pass at `level` (i3d_debug_track_sums: 29 sums; i3d_debug_track_rgbd_sums: 31, the photometric r^2 and sample count appended)
int track_sums_run(const Model& m, const i3d_track_desc* d, int32_t w, int32_t h, const float* depth, int32_t level, const double* pose_ref6, const double* pose_cur6,
                   double* sums, int64_t* inliers, TrackRgbd* rgbd = nullptr);

// the point query: validation, the scratch (points, the requested outputs, the rows), the launches, the copies back and the one synchronisation
int query_run(const Model& m, const i3d_query_desc* d, int64_t n, const double* points, double* sdf, float* normal, float* albedo, double* foot, double* distance,
              uint8_t* status, i3d_query_stats* stats);

// the caller's own rays: validation, the bitmap, the scratch (rays, ranges, the requested outputs, with order = 1 the keys, the permutation
// and the sort's storage, the stats), the launches, the copies back and the one synchronisation.  albedo / shading / intensity: null for a model without them;
// have_sh: the per-voxel SH that shading / intensity read is there.  colour_call: the colour call of DESIGN.md 35 (Model::cast_rays_color), which has t, status
// and color [n][3] alone; otherwise color is not read
int cast_rays_run(const Model& m, bool have_sh, int32_t order, int64_t n, const double* origins, const double* directions, const double* t_min, const double* t_max, double* t,
                  double* position, float* normal, float* albedo, float* shading, float* intensity, uint8_t* status, i3d_render_stats* stats,
                  bool colour_call = false, float* color = nullptr);

// rotation (row-major) -> angle-axis, stable at small angles and near pi (track.cpp)
void rot_to_aa(const double R[9], double aa[3]);
// a camera -> world pose, and its conversions from / to the world -> camera angle-axis | t of i3d_set_camera / the renderer (track.cpp)
struct Pose { double R[9], t[3]; };
Pose pose_from_vec6(const double* p6);
void vec6_from_pose(const Pose& P, double* p6);

// the point-set registration: validation, the scratch (points, slab, state), then register_loop; two stream synchronisations.  debug_pivot3 != null:
// one pass at pose6_io about that pivot, its 29 sums and valid count (i3d_debug_register_sums)
int register_run(const Model& m, const i3d_register_desc* d, int64_t n, const double* points, double* pose6_io, i3d_register_stats* stats,
                 const double* debug_pivot3 = nullptr, double* debug_sums29 = nullptr, int64_t* debug_valid = nullptr);

// The loop of sections 18 and 28, from the pivot to the filled result, over whatever the two launchers read their points from: the pivot by a mean pass and
// k_track_solve, the start state, the budget launched back to back, the totals at the returned pose, the figures, and the rule that a call which applied no step
// leaves pose6_io bit for bit.  Two stream synchronisations (one with debug_pivot3: one pass at pose6_io about that pivot, its 29 sums and valid count, out untouched)
struct RegisterLoop {
    double* slab; TrackState* state;                                                           // [register_rows(n, per_lane)][TRACK_COLS], and the device state
    long long n; int per_lane;
    std::function<void(const double* R0, const double* t0)> mean;                              // the mean pass about the start pose into slab
    std::function<void(const RegisterParams& p, int check_done)> pass;                         // one pass at the pose of state into slab
    int iterations; double stop_rotation, stop_translation, max_distance;
    const double* debug_pivot3 = nullptr; double* debug_sums29 = nullptr; int64_t* debug_valid = nullptr;
};
int register_loop(const Model& m, const RegisterLoop& lp, double* pose6_io, i3d_register_stats& out);      // of m: the stream and fail

// the pivot c = R0 mean(p) + t0 from the totals of a mean pass (columns 0..2 the sum, 3 the number), and the state a loop starts from: the start pose about the
// pivot (register.cpp; sections 18 and 19 share them)
void pivot_of(const double* sums, const double* R0, const double* t0, double* c);
void start_state(TrackState& hs, const double* R0, const double* t0, const double* c);

// the photometric term of i3d_track_frame_sdf_rgbd: its inputs and where its results go.  stats: one per frame of the call (may be null)
struct TrackSdfRgbd {
    double geometric_weight, photo_weight; float max_photo_residual;
    i3d_track_sdf_rgbd_stats* stats = nullptr;
};
inline TrackSdfRgbd rgbd_of(const i3d_track_sdf_rgbd_desc* d, i3d_track_sdf_rgbd_stats* stats) {
    return TrackSdfRgbd{d->geometric_weight, d->photo_weight, d->max_photo_residual, stats};
}
// the frames of a call, all w x h.  host_depth: the images [num][h][w], uploaded chunk by chunk; null: dev_depth[num] are resident device images and nothing
// is uploaded.  The luminance likewise (read with a TrackSdfRgbd only)
struct TrackSdfFrames {
    int32_t num, w, h;
    const float* host_depth; const float* const* dev_depth;
    const float* host_lum; const float* const* dev_lum;
};
// one pass at a given pivot instead of a registration (the i3d_debug_*_sums entry points): its sums - 29, with a TrackSdfRgbd 31, the photometric r^2 and sample
// count appended - and the counts that are asked for
struct TrackSdfDebug { const double* pivot3; double* sums; int64_t* valid; int64_t* usable; int64_t* photo_samples; };
// The one driver, after the caller's checks: the frames of fr under the camera intr / dist from the poses of poses6_io (world -> camera; the loop runs on the
// inverse), at most max_chunk at a time (<= 0: as many as the scratch rule allows).  Per chunk: the upload, the pivot pass and solve, one synchronisation, the
// pivots and start states formed on the host, the whole budget launched back to back, the figures pass, one read-back and a second synchronisation.  With a
// TrackSdfRgbd: the luminance beside the depth, the intensity volume filled once before the first pivot pass, the combined system.  debug (one frame): no pivot
// pass, a budget of 0, the sums handed back and the pose left alone
int track_sdf_chunks(const Model& m, const i3d_track_sdf_desc* d, const double* intr, const double* dist, const TrackSdfFrames& fr, double* poses6_io,
                     i3d_track_sdf_stats* stats, const TrackSdfRgbd* rgbd = nullptr, int max_chunk = 0, const TrackSdfDebug* debug = nullptr);
// a single frame: the validation of DESIGN.md 19 (with rgbd: 21), then track_sdf_chunks with one frame
int track_sdf_run(const Model& m, const i3d_track_sdf_desc* d, int32_t w, int32_t h, const float* depth, double* pose6_io, i3d_track_sdf_stats* stats,
                  const TrackSdfRgbd* rgbd = nullptr, const float* luminance = nullptr, const TrackSdfDebug* debug = nullptr);

}  // namespace i3d
