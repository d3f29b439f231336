// Host-side state of one device context: resident voxel grid, keyframes, camera model, row storage and solver vectors.
#pragma once
#include <functional>
#include <string>
#include <vector>
#include <cstring>
#include <cmath>
#include "../device/kernels.hpp"
#include "comm.hpp"
#include "model.hpp"

namespace i3d {

// The I3D_* environment switches of the solver and its kernels, parsed in ONE place (read_switches, solver.cpp) at the top of every assemble and at the entry of
// the other public calls that need one (estimate_sh): a switch takes effect at the next outer iteration or call, none is cached per process.  (The communicator's
// I3D_TRANSPORT / I3D_SIM_P2P / I3D_FORCE_COLLECTIVES are read when it is created, comm.cpp / capi.cpp.)
struct SolverSwitches {
    int  deterministic = -1;        // I3D_DETERMINISTIC: -1 unset (on for one rank, off when sharded), else 0 / 1
    int  ladder = LADDER_MAX;       // I3D_LADDER, clamped to [1, LADDER_MAX]
    bool ladder_mr = true, ladder_mr1 = false, ladder_pair = true; int ladder_group = 3;      // I3D_LADDER_MR / _MR1 / _PAIR / _GROUP
    bool egt_mr1 = false;           // I3D_EGT_MR1
    int  egt_tile = 0;              // I3D_EGT_TILE: 0 unset, else 512 or 1024
    int  hmax_limit = 0, hmax_limit_1024 = 0;      // I3D_EGT_HMAX_LIMIT, I3D_EGT_HMAX_LIMIT_1024 (0: none)
    bool halo_pull = false, no_tile = false, gradcol = true, cost0 = true;      // I3D_HALO_PULL, I3D_NO_TILE, I3D_GRADCOL, I3D_COST0
    int  no_cull = 0;               // I3D_NO_CULL: 0 .. 3
    int  debug_invalid_attempt = -1;      // I3D_DEBUG_INVALID_ATTEMPT
    int  sh_slab = 0;               // I3D_SH_SLAB (0: the default cap)
};

// Which operator pass an outer iteration plans for and on which tile geometry: filled once per assemble (plan_operator, assemble.cpp, where the reasons stand), the
// overflow fall-backs applied by plan_other_geometry / settle_plan; read by tile_plan() and by the route of the solve (SolveRoute, solver_internal.hpp)
struct OperatorPlan {
    bool deterministic = false;     // bit-reproducible operator pass (default on one rank, I3D_DETERMINISTIC=0 / =1 override)
    int  ladder_max = 1;            // I3D_LADDER where the ladder can run: attempts solved together, 1 = the serial loop
    bool mr1_serial = false;        // I3D_EGT_MR1=1: the serial loop's operator pass is k_eg_tile_mr<1> (A/B runs, the control of the ladder tests)
    bool ladder_lists = false;      // the pull lists are built for the multi-system operator pass (tile_pass_mr.hip) although the single-system pass pushes its halo
    bool halo_pull = false;         // halo sums pulled over the plan's lists (tile_pass.hip k_tile_pull_plan): I3D_HALO_PULL=1 and the bit-reproducible mode
    int  tile_T = 0;                // geometry of the current plan (0 = the default, 1024); single rank: 512 when a 1024-entry tile's halo does not fit; sharded: 512 first, then 1024
    bool tile_ok = false;           // the plan fits its halo slots (false: the untiled pass, single rank only)
    bool pull_lists() const { return halo_pull || ladder_lists; }
};

// Sharding (assemble.cpp shard_plan; see common.hpp): owned range / compute list of this rank, the halo exchange plan of the current work list
// (shard_kernels.hip) and the foreign tiles with ghost entries
struct ShardState {
    int chunk = 1, own0 = 0, own1 = 0, nC = 0, slice = 0, n_ghost_tiles = 0;
    DevBuf<int> clist, cflag, cscan;
    HaloPlan halo; DevBuf<unsigned long long> need_mask, halo_items, halo_sorted;
    DevBuf<int> halo_count, halo_send_idx, halo_recv_idx, halo_send_peer, halo_recv_peer, halo_offs, tile_flag, ghost_tiles;
    DevBuf<float> halo_send_buf, halo_recv_buf; DevBuf<unsigned char> halo_temp;
};

// The damping ladder (solver.cpp lm_solve / pcg.cpp pcg_solve_ladder): per-system slabs of the PCG vectors and partial sums, and its counters
struct LadderState {
    int hint = 0, hint_prev = 0;    // LM attempts of the last two outer iterations (the first batch speculates as deep as the larger)
    LadVec strides{};               // strides of the slabs below
    DevBuf<float> vec;              // [LADDER_MAX][6][strides.vec]: x, r, p, z, u, qacc of every system
    DevBuf<float> qh, cam, mblk, tail;
    DevBuf<double> part;            // [LADDER_MAX][strides.part]: the partial sums of a system (Partials, pcg.cpp)
    DevBuf<double> red;             // sharded ladder: what a pass all-reduces — [LADDER_MAX][4] slice sums | [LADDER_MAX][6K + 10, padded] camera block + p.q
    DevBuf<PcgState> st;            // [LADDER_MAX][2]
    long long batches = 0, streams = 0, system_passes = 0, resyncs = 0, wasted = 0;      // counters (i3d_debug_ladder_stats)
    long long pass_live[7] = {0, 0, 0, 0, 0, 0, 0}, paired = 0;                          // operator passes by live systems, paired launches (i3d_debug_ladder_passes)
};

struct Timing {
    bool on = false;
    unsigned mask = ~0u;                            // categories that get HIP events (an event pair per launch is not free: ~8 % with all of them on)
    double ms[I3D_K_COUNT] = {0};
    long long launches[I3D_K_COUNT] = {0};
    std::vector<float> each[I3D_K_COUNT];          // every launch duration (for the work-only average)
    struct Pending { hipEvent_t a, b; int cat; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> pool;
};

}  // namespace i3d

struct i3d_context {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    // ---- grid (device order = brick-Morton sorted) ----
    int N = 0; float voxel_size = 0, truncation = 0;
    i3d::DevBuf<int> cx, cy, cz, rank, nbr, aidx, alist, aflag, ascan;
    i3d::DevBuf<double> sdf0, x_sdf, x_alb, xc_sdf, xc_alb;
    i3d::DevBuf<float> f_sdf, f_alb, weight, sh;
    i3d::DevBuf<uchar4> color;
    i3d::DevBuf<uint8_t> flags;
    i3d::DevBuf<unsigned char> scan_tmp; size_t scan_tmp_bytes = 0;
    i3d::DevBuf<unsigned long long> hkeys; i3d::DevBuf<int> hvals; unsigned int hmask = 0;     // device hash of the resident grid (kept for the level kernels)
    bool have_grid = false, have_sh = false;
    // what the drivers that read the stored field keep between calls (model.hpp); set_grid_device drops its brick bitmap.  The two debug knobs of those
    // drivers: the slab row cap and the frames per chunk of the batch trackers (<= 0: the default rule); tests lower them
    i3d::ModelBuffers model; int register_row_cap = i3d::REGISTER_MAX_ROWS, track_batch_frames = 0;
    // the lighting estimate behind `sh` (LightingSVSH::subvolumes() / shCoeffs()): packed subvolume indices (ascending), nine coefficients each, the subvolume size —
    // what the "shading" colour modes of the mesh export interpolate at every voxel (SDFVisualization::applyColorShading)
    std::vector<unsigned long long> sv_keys; std::vector<double> sv_sh; float sv_size = 0.0f; bool have_subvolumes = false;

    // ---- keyframes ----
    int K = 0, levels = 0;
    std::vector<int> fw, fh;                        // per level
    std::vector<i3d::DevBuf<float>> lum, depth;     // [K*levels]
    std::vector<i3d::DevBuf<uint8_t>> bgr;
    i3d::DevBuf<i3d::FrameConst> d_frames, d_frames_cand;
    bool have_frames = false;

    // ---- camera (fp64 master copy on the host) ----
    double intr[4] = {0, 0, 0, 0}, dist[5] = {0, 0, 0, 0, 0};
    std::vector<double> poses;
    bool have_camera = false;

    // ---- rows (work-list space) ----
    int Acap = 0, slots = 0, A = 0; long long n_active = 0;
    i3d::Comm* comm = nullptr; i3d::ShardState shard;
    bool sharded() const { return comm && (comm->world > 1 || comm->force); }      // the sharded code path and its collectives (one forced rank runs them too)
    i3d::DevBuf<int> obs_frame, anbr; i3d::DevBuf<float> obs_w, ea_w, C, treg;
    i3d::DevBuf<float4> rows; i3d::DevBuf<float2> row_wr;
    i3d::DevBuf<uint8_t> aflags, nrows, regflags, ea_free; i3d::DevBuf<int> gmax;
    // culling in front of the observation pass (cull_kernels.hip): 8x8-block depth ranges of every keyframe at level cull_level (-1: not built), bounding spheres and
    // keyframe masks of the 64-entry groups of the compute list
    i3d::DevBuf<float2> cull_blocks; i3d::DevBuf<float4> cull_bounds; i3d::DevBuf<unsigned> cull_mask; int cull_level = -1; bool cull_on = false;
    // tiled operator pass (tile_pass.hip): plan of the current work list
    double cost_at_build = 0.0;       // 0.5 sum_t type_w[t] sum(w r^2) at the point the rows were built at (assemble)
    i3d::DevBuf<float> C2, treg2, gc_part;      // the second set of staging planes + the camera rows of the one-stream gradient / column-norm pass (gradcol.hip)
    i3d::DevBuf<float> aux_part;      // one float row of camera totals per workgroup of the gradient / column-norm passes (summed in a fixed order)
    i3d::DevBuf<unsigned> tp_lnbr; i3d::DevBuf<int> tp_halo_idx, tp_halo_cnt, tp_iota, tp_ext_e, tp_ext_pos, tp_ext_off, tp_overflow; i3d::DevBuf<float> tp_qh, tp_eaw, cam_part;
    i3d::DevBuf<unsigned char> tp_temp;
    i3d::DevBuf<unsigned short> tp_hp_off, tp_hp_src;      // halo pull lists of the plan (OperatorPlan::pull_lists)
    i3d::SolverSwitches sw;         // the environment switches as of the last assemble / estimate_sh (read_switches)
    i3d::OperatorPlan op;           // set at every assemble
    i3d::LadderState ladder;
    double t_add_end = 0.0;         // host clock at the end of the residual collection of the current outer iteration (time_add | time_build)
    int plan_T() const { return op.tile_T > 0 ? op.tile_T : (sw.egt_tile == 512 ? 512 : 1024); }
    int plan_hmax_limit() const { return plan_T() == 512 ? sw.hmax_limit : sw.hmax_limit_1024; }      // tests of the overflow handling
    i3d::TilePlan tile_plan() const {
        const int T = plan_T();
        const bool sh = sharded();
        const int t0 = sh ? shard.own0 / T : 0, t1 = sh ? (shard.own1 + T - 1) / T : i3d::tile_plan_tiles_of(A, T);
        return i3d::TilePlan{tp_lnbr.p, tp_eaw.p, tp_halo_idx.p, tp_halo_cnt.p, tp_iota.p, tp_ext_e.p, tp_ext_pos.p, tp_qh.p, tp_ext_off.p, tp_overflow.p, T, i3d::tile_plan_hmax_of(T), t0, t1 > t0 ? t1 - t0 : 0,
                             shard.ghost_tiles.p, sh ? shard.n_ghost_tiles : 0, op.deterministic ? 1 : 0, op.pull_lists() ? tp_hp_off.p : nullptr, op.pull_lists() ? tp_hp_src.p : nullptr, op.halo_pull ? 1 : 0};
    }

    // ---- solver vectors (length NP = 2N + 6K + 9) ----
    i3d::DevBuf<float> v_mask, v_c, v_S, v_cm, v_D2, v_Minv, v_b, v_x, v_r, v_p, v_z, v_q, v_u, v_acc, v_tmp, v_qacc;
    i3d::DevBuf<float> Minv_blocks;
    i3d::DevBuf<double> d_shared, d_blocks, d_scal, d_xshared, d_xcshared;
    i3d::DevBuf<i3d::PcgState> d_pcg, d_pcg2; i3d::DevBuf<double> d_partials;
    int* h_flags = nullptr; int* d_flags = nullptr; int pcg_seq = 1024;      // pinned (seq, done) ring written by k_pcg_tail_a, polled by the host
    // the trust-region loop on the device (lm_kernels.hip): its state, one record per attempt in mapped host memory, the camera blocks of J^T W J it damps
    i3d::DevBuf<i3d::LmState> d_lm; i3d::LmRecord* h_lmrec = nullptr; i3d::LmRecord* d_lmrec = nullptr; int lm_seq = 1;
    i3d::DevBuf<double> d_cam_c, d_cam_H;
    hipEvent_t ev_asm[2] = {nullptr, nullptr};      // start of an outer iteration's assembly | end of its residual collection (time_add / time_build without a synchronisation)
    long long n_syncs = 0;                          // hipStreamSynchronize calls of the solver path (i3d_debug_sync_count)
    double* h_pinned = nullptr; size_t h_pinned_n = 0;

    i3d::OptParams last_params; bool assembled = false;
    long long last_sizes[6] = {0, 0, 0, 0, 0, 0};
    i3d::Timing timing;

    // views
    i3d::GridView grid_view() const;
    i3d::RowView row_view() const;
};

namespace i3d {

// helpers implemented in context.cpp
int ctx_fail(i3d_context* c, int code, const std::string& msg);
int ctx_hip(i3d_context* c, hipError_t e, const char* what);
int ctx_launch_check(i3d_context* c);      // hipGetLastError + the latched launch-configuration error (common.hpp: set_dynamic_lds) -> I3D_ERR_HIP / I3D_ERR_CAPACITY
#define CTX_HIP(c, expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return i3d::ctx_hip((c), _e, #expr); } while (0)
void build_frame_consts(const i3d_context* c, int level, const double* poses, std::vector<FrameConst>& out);
int ensure_pinned(i3d_context* c, size_t n);
bool timing_begin(i3d_context* c, int cat);
void timing_end(i3d_context* c);
void timing_flush(i3d_context* c);
struct TimedScope { i3d_context* c; bool active; TimedScope(i3d_context* c_, int cat) : c(c_), active(timing_begin(c_, cat)) {} ~TimedScope() { if (active) timing_end(c); } };

// What every extern "C" function with a context does first: its answer to a null handle — each entry point keeps its own, a bare code or ctx_fail's, shared
// with the first validation `valid` that answers the same (`true`: none does) — then the context's device.
#define CTX_ENTER(c, valid, refusal) do { if (!(c) || !(valid)) return (refusal); CTX_HIP((c), hipSetDevice((c)->device)); } while (0)

// Every upload and readback of a context goes on its stream: the stream is non-blocking, so a blocking hipMemcpy is not ordered against what is queued on it.
// Both only queue the copy; ctx_sync ends a call's downloads (one synchronisation for all of them) and stands before host memory of an upload goes out of scope.
template <class T> hipError_t ctx_upload(i3d_context* c, T* dev, const T* host, size_t n) { return hipMemcpyAsync(dev, host, sizeof(T) * n, hipMemcpyHostToDevice, c->stream); }
template <class T> hipError_t ctx_download(i3d_context* c, T* host, const T* dev, size_t n) { return hipMemcpyAsync(host, dev, sizeof(T) * n, hipMemcpyDeviceToHost, c->stream); }
inline hipError_t ctx_sync(i3d_context* c) { return hipStreamSynchronize(c->stream); }

// A grid in the caller's visit order on the device: the six arrays a caller hands over (i3d_grid_view) and takes back (i3d_export_grid), and what the level
// transitions rebuild the resident grid from (grid_io.cpp set_grid_device)
struct GridStaging {
    DevBuf<int> kxyz; DevBuf<double> sdf, sdf_ref, alb; DevBuf<float> w; DevBuf<uint8_t> rgb;
    hipError_t alloc(size_t n) {
        for (hipError_t e : {kxyz.alloc(3 * n), sdf.alloc(n), sdf_ref.alloc(n), alb.alloc(n), w.alloc(n), rgb.alloc(3 * n)}) if (e != hipSuccess) return e;
        return hipSuccess;
    }
    VisitView view() const { return VisitView{kxyz.p, sdf.p, sdf_ref.p, alb.p, w.p, rgb.p}; }
};
int set_grid_device(i3d_context* c, int N, float voxel_size, float truncation, GridStaging& st);

// The crossing between device order and the caller's visit order on the host (context.cpp): rank (device slot -> visit index) and, where wanted, the work list
// of the last assembly (entry -> device slot).  fetch() queues the downloads once per call; they are there after the caller's ctx_sync / sync_stream.
struct VisitOrder {
    std::vector<int> rank, alist;
    int fetch(i3d_context* c, bool work_list);
    int of_entry(int a) const { return rank[alist[a]]; }
    // a solver vector on the device ([sdf chunk | albedo chunk | camera], single-rank layout) -> [sdf N | albedo N | camera] in visit order; synchronises
    int vector_to_visit(i3d_context* c, const float* dev_vec, double* out);
};
// visit index -> device slot, into a scratch buffer of the call (not resident: 4 bytes per voxel that only the transitions, the export and the mesh read)
int inverse_rank(i3d_context* c, DevBuf<int>& inv);
// the total of an exclusive scan of n flags / counts: its last element + the last input, queued behind the scan; total() after the next synchronisation
struct ScanTotal {
    int tail[2] = {0, 0};
    hipError_t queue(i3d_context* c, const int* in, const int* scan, int n) {
        if (n <= 0) return hipSuccess;
        const hipError_t e = ctx_download(c, &tail[0], scan + (n - 1), 1);
        return e != hipSuccess ? e : ctx_download(c, &tail[1], in + (n - 1), 1);
    }
    long long total() const { return (long long)tail[0] + tail[1]; }
};
// size of pyramid level l of a w x h image: every level halves the one below, rounding down (Pyramid::create)
inline void level_size(int w, int h, int l, int& lw, int& lh) { lw = w; lh = h; for (int i = 0; i < l; ++i) { lw /= 2; lh /= 2; } }
// the camera half of OptParams at a pyramid level (optimizer.cpp:125; Camera::setIntrinsics(Vec4) casts to float, camera.cpp:95-98); the rest stays zero
OptParams camera_params(const i3d_context* c, int level, float occlusion);
inline double varying_lambda(int it, int n, double l0, double l1) { return n <= 1 ? l0 : l0 + ((l1 - l0) / (double)(n - 1)) * (double)it; }      // cost.h:130-143

// the grid as the kernels that sample the field at points read it: no brick bitmap, nothing marches; and as the ray caster reads it, with the cached bitmap
inline RenderGrid field_grid(const i3d_context* c, bool refined) {
    return RenderGrid{HashTable{c->hkeys.p, c->hvals.p, c->hmask}, c->nbr.p, c->N, c->weight.p, refined ? c->x_sdf.p : c->sdf0.p, c->x_alb.p, c->sh.p,
                      (double)c->voxel_size, nullptr, {0, 0, 0}, {0, 0, 0}, c->color.p};
}
inline RenderGrid render_grid(const i3d_context* c, bool refined) {
    RenderGrid g = field_grid(c, refined);
    const ModelBuffers::Bricks& k = c->model.bricks;
    g.bits = k.bits.p;
    for (int a = 0; a < 3; ++a) { g.lo[a] = k.lo[a]; g.dim[a] = k.dim[a]; }
    return g;
}

// the context as a model (model.hpp): fn names the entry point in the messages, refined chooses the field
struct ContextModel final : Model {
    i3d_context* c; bool refined;
    ContextModel(i3d_context* c_, const std::string& fn_, bool refined_)
        : Model(c_->model, c_->device, c_->stream, (double)c_->voxel_size, c_->register_row_cap, "grid", "i3d_render_view", true, fn_), c(c_), refined(refined_) {}
    int fail(int code, const std::string& msg) const override { return ctx_fail(c, code, msg); }
    int check_state(bool use_context_camera, const double*& intr, const double*& dist) const override {
        if (!c->have_grid) return fail(I3D_ERR_STATE, fn + ": no grid");
        if (use_context_camera) {
            if (!c->have_camera) return fail(I3D_ERR_STATE, fn + ": use_context_camera without a camera (i3d_set_camera)");
            intr = c->intr; dist = c->dist;
        }
        return I3D_OK;
    }
    int intensity_ready() const override {
        return c->have_sh ? I3D_OK : fail(I3D_ERR_STATE, fn + ": a photometric weight > 0 needs the per-voxel SH (i3d_set_voxel_sh / i3d_estimate_sh)");
    }
    size_t intensity_entries() const override { return (size_t)c->N; }
    void launch_intensity(double* vol) const override { launch_voxel_intensity(stream, field_grid(c, refined), vol); }
    void brick_bounds(int* bounds) const override { launch_render_brick_bounds(stream, c->N, c->cx.p, c->cy.p, c->cz.p, c->weight.p, bounds); }
    void brick_fill(unsigned* bits, const int lo[3], const int dim[3]) const override {
        launch_render_brick_fill(stream, c->N, c->cx.p, c->cy.p, c->cz.p, c->weight.p, bits, lo, dim);
    }
    void cast(const RenderCam& cam, const RenderPlanes& out, RenderStatsDev* stats) const override { launch_render(stream, render_grid(c, refined), cam, out, stats); }
    void cast_rays(const CastRays& p, RenderStatsDev* stats) const override { launch_cast_rays(stream, render_grid(c, refined), p, stats); }
    void cast_color(const RenderCam& cam, const RenderColorPlanes& out, RenderStatsDev* stats) const override {
        launch_render_color(stream, render_grid(c, refined), cam, out, stats);
    }
    void cast_rays_color(const CastRaysColor& p, RenderStatsDev* stats) const override { launch_cast_rays_color(stream, render_grid(c, refined), p, stats); }
    void query(const QueryParams& p, const double* points, const QueryOut& out, QueryRow* rows, QueryRow* total) const override {
        launch_query(stream, field_grid(c, refined), p, points, out, rows, total);
    }
    void register_pass(const RegisterParams& p, const double* points, const TrackState* state, int check_done, double* slab) const override {
        launch_register(stream, field_grid(c, refined), p, points, state, check_done, slab);
    }
    void track_sdf_pass(const TrackSdfParams& p, const TrackSdfPhoto* ph, const TrackSdfBatch& b, int check_done) const override {
        launch_track_sdf(stream, field_grid(c, refined), p, ph, b, check_done);
    }
};

// levels.cpp (their extern "C" callers have entered the context: CTX_ENTER)
int recompute_colors(i3d_context* c, float occlusion_distance, int num_observations);
int clear_outside_thin_shell(i3d_context* c, double thres_shell, int64_t* new_count);
int upsample_grid(i3d_context* c, int64_t* new_count);

// solver.cpp (the stages it drives: assemble.cpp, pcg.cpp; what they share: solver_internal.hpp)
void read_switches(i3d_context* c);      // the environment -> c->sw
int assemble(i3d_context* c, const i3d_optimizer_config& cfg, int iteration, OptParams& p, i3d_iteration_stats* st);      // assemble.cpp
int optimize(i3d_context* c, const i3d_optimizer_config& cfg, i3d_iteration_stats* stats);

// lighting.cpp
int estimate_sh(i3d_context* c, float subvolume_size, double lambda_reg, double thres_shell, int* num_subvolumes, double* sh,
                int32_t* sub_index, int cap, i3d_sh_stats* stats);

}  // namespace i3d
