// Context lifetime, errors, timing, the device views, per-keyframe constants, and what the files of the context layer share (context.hpp): the crossing between
// device order and visit order, the inverse rank, the camera half of OptParams.  Grid in and out: grid_io.cpp; keyframes and camera: frames.cpp.
#include "context.hpp"
#include "../device/frame_math.hpp"
#include "../device/level_kernels.hpp"
#include <algorithm>

using namespace i3d;

static thread_local std::string g_create_error;

namespace i3d {

int ctx_fail(i3d_context* c, int code, const std::string& msg) { if (c) c->err = msg; else g_create_error = msg; return code; }
int ctx_hip(i3d_context* c, hipError_t e, const char* what) {
    return ctx_fail(c, I3D_ERR_HIP, std::string(what) + " -> " + hipGetErrorString(e));
}

int ctx_launch_check(i3d_context* c) {
    char msg[256];
    if (take_launch_error(msg, sizeof(msg))) return ctx_fail(c, I3D_ERR_CAPACITY, msg);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? I3D_OK : ctx_hip(c, e, "kernel launch");
}

int ensure_pinned(i3d_context* c, size_t n) {
    if (n <= c->h_pinned_n) return I3D_OK;
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    c->h_pinned = nullptr; c->h_pinned_n = 0;
    CTX_HIP(c, hipHostMalloc((void**)&c->h_pinned, n * sizeof(double), hipHostMallocDefault));
    c->h_pinned_n = n;
    return I3D_OK;
}

// ---- timing: one HIP event pair per launch on the context's stream, resolved at flush -------------------------
bool timing_begin(i3d_context* c, int cat) {
    if (!c->timing.on || !((c->timing.mask >> cat) & 1u)) return false;
    Timing::Pending p; p.cat = cat;
    auto get = [&]() { hipEvent_t e; if (!c->timing.pool.empty()) { e = c->timing.pool.back(); c->timing.pool.pop_back(); } else (void)hipEventCreate(&e); return e; };
    p.a = get(); p.b = get();
    (void)hipEventRecord(p.a, c->stream);
    c->timing.pending.push_back(p);
    return true;
}
void timing_end(i3d_context* c) {
    if (c->timing.pending.empty()) return;
    (void)hipEventRecord(c->timing.pending.back().b, c->stream);
}
void timing_flush(i3d_context* c) {
    if (c->timing.pending.empty()) return;
    (void)hipStreamSynchronize(c->stream);
    for (auto& p : c->timing.pending) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) { c->timing.ms[p.cat] += ms; c->timing.launches[p.cat] += 1; c->timing.each[p.cat].push_back(ms); }
        c->timing.pool.push_back(p.a); c->timing.pool.push_back(p.b);
    }
    c->timing.pending.clear();
}

// ---- per-keyframe constants ------------------------------------------------------------------------------------
// (the formulas live in device/frame_math.hpp: the device builds the same constants for the candidate point of every LM attempt)
void build_frame_consts(const i3d_context* c, int level, const double* poses, std::vector<FrameConst>& out) {
    out.resize(c->K);
    for (int f = 0; f < c->K; ++f) {
        FrameConst& fc = out[f];
        fm::frame_from_pose(poses + 6 * f, fc);
        const size_t k = (size_t)f * c->levels + level;
        fc.hot.lum = c->lum[k].p; fc.depth = c->depth[k].p; fc.bgr = c->bgr[k].p;
        fc.w = c->fw[level]; fc.h = c->fh[level];
    }
}

// ---- device order <-> visit order -----------------------------------------------------------------------------
int VisitOrder::fetch(i3d_context* c, bool work_list) {
    rank.resize(c->N); alist.resize(work_list && c->A > 0 ? c->A : 0);
    CTX_HIP(c, ctx_download(c, rank.data(), c->rank.p, rank.size()));
    if (!alist.empty()) CTX_HIP(c, ctx_download(c, alist.data(), c->alist.p, alist.size()));
    return I3D_OK;
}
int VisitOrder::vector_to_visit(i3d_context* c, const float* dev_vec, double* out) {
    const int N = c->N, A = c->A, K = c->K, NS = 6 * K + 9, ch = c->shard.chunk, NP = 2 * ch + NS;
    std::vector<float> h(NP);
    CTX_HIP(c, ctx_download(c, h.data(), dev_vec, h.size()));
    CTX_HIP(c, ctx_sync(c));
    for (int i = 0; i < 2 * N + NS; ++i) out[i] = 0.0;
    for (int a = 0; a < A; ++a) { const int v = of_entry(a); out[v] = h[a]; out[N + v] = h[ch + a]; }
    for (int i = 0; i < NS; ++i) out[2 * N + i] = h[2 * ch + i];
    return I3D_OK;
}
int inverse_rank(i3d_context* c, DevBuf<int>& inv) {
    CTX_HIP(c, inv.alloc(c->N));
    launch_inv_rank(c->stream, c->N, c->rank.p, inv.p);
    return I3D_OK;
}

OptParams camera_params(const i3d_context* c, int level, float occlusion) {
    OptParams p; std::memset(&p, 0, sizeof(p));
    p.K = c->K; p.level = level; p.occlusion = occlusion;
    p.pyr_scale = 1.0 / std::pow(2.0, level);                      // cost.h:146-150
    for (int i = 0; i < 4; ++i) { p.intr[i] = c->intr[i]; p.cam_f[i] = (float)(c->intr[i] * p.pyr_scale); }
    bool dz = true;
    for (int i = 0; i < 5; ++i) { p.dist[i] = c->dist[i]; p.dist_f[i] = (float)c->dist[i]; if (std::fabs(p.dist_f[i]) > 1e-5f) dz = false; }
    p.dist_zero = dz ? 1 : 0;
    p.w = c->fw[level]; p.h = c->fh[level];
    return p;
}

}  // namespace i3d

i3d::GridView i3d_context::grid_view() const {
    GridView g;
    g.N = N; g.voxel_size = voxel_size; g.truncation = truncation;
    g.cx = cx.p; g.cy = cy.p; g.cz = cz.p; g.rank = rank.p; g.nbr = nbr.p; g.weight = weight.p; g.color = color.p;
    g.sdf0 = sdf0.p; g.x_sdf = x_sdf.p; g.x_alb = x_alb.p; g.f_sdf = f_sdf.p; g.f_alb = f_alb.p; g.sh = sh.p;
    g.flags = flags.p; g.aidx = aidx.p;
    return g;
}
i3d::RowView i3d_context::row_view() const {
    RowView r;
    r.A = A; r.Acap = Acap; r.slots = slots; r.chunk = shard.chunk; r.world = comm ? comm->world : 1; r.own0 = shard.own0; r.own1 = shard.own1;
    r.clist = sharded() ? shard.clist.p : nullptr; r.nC = shard.nC; r.alist = alist.p; r.aflags = aflags.p; r.anbr = anbr.p; r.obs_frame = obs_frame.p; r.obs_w = obs_w.p;
    r.rows = rows.p; r.row_wr = row_wr.p; r.nrows = nrows.p; r.gmax = gmax.p; r.regflags = regflags.p; r.ea_w = ea_w.p; r.ea_free = ea_free.p;
    return r;
}

extern "C" {

const char* i3d_version(void) { return "intrinsic3d_hip 0.1 (gfx950)"; }
const char* i3d_last_error(const i3d_context* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int i3d_create(int32_t device_ordinal, i3d_context** out) {
    if (!out) return ctx_fail(nullptr, I3D_ERR_INVALID_ARGUMENT, "i3d_create: null output pointer");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return ctx_fail(nullptr, I3D_ERR_NO_DEVICE, "no HIP device visible: this library has no CPU fallback");
    if (device_ordinal < 0 || device_ordinal >= count) return ctx_fail(nullptr, I3D_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    e = hipSetDevice(device_ordinal);
    if (e != hipSuccess) return ctx_hip(nullptr, e, "hipSetDevice");
    auto* c = new i3d_context();
    c->device = device_ordinal;
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return ctx_hip(nullptr, e, "hipStreamCreate"); }
    *out = c;
    return I3D_OK;
}

void i3d_destroy(i3d_context* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    timing_flush(c);
    for (auto e : c->timing.pool) (void)hipEventDestroy(e);
    if (c->h_pinned) (void)hipHostFree(c->h_pinned);
    if (c->h_flags) (void)hipHostFree(c->h_flags);
    if (c->h_lmrec) (void)hipHostFree(c->h_lmrec);
    for (auto e : c->ev_asm) if (e) (void)hipEventDestroy(e);
    delete c->comm;
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int i3d_timing_enable(i3d_context* c, int32_t on) { CTX_ENTER(c, true, I3D_ERR_INVALID_ARGUMENT); timing_flush(c); c->timing.on = on != 0; return I3D_OK; }
int i3d_timing_select(i3d_context* c, uint32_t category_mask) { CTX_ENTER(c, true, I3D_ERR_INVALID_ARGUMENT); timing_flush(c); c->timing.mask = category_mask; return I3D_OK; }
int i3d_timing_get(i3d_context* c, double* ms, int64_t* launches, int32_t reset) {
    CTX_ENTER(c, true, I3D_ERR_INVALID_ARGUMENT);
    timing_flush(c);
    for (int i = 0; i < I3D_K_COUNT; ++i) { if (ms) ms[i] = c->timing.ms[i]; if (launches) launches[i] = c->timing.launches[i]; }
    if (reset) for (int i = 0; i < I3D_K_COUNT; ++i) { c->timing.ms[i] = 0; c->timing.launches[i] = 0; c->timing.each[i].clear(); }
    return I3D_OK;
}
int i3d_timing_get_work(i3d_context* c, double* ms, int64_t* launches) { return i3d_timing_get_work_ex(c, ms, launches, nullptr, nullptr); }
int i3d_timing_get_work_ex(i3d_context* c, double* ms, int64_t* launches, double* slow_ms, int64_t* slow_launches) {
    CTX_ENTER(c, true, I3D_ERR_INVALID_ARGUMENT);
    timing_flush(c);
    for (int i = 0; i < I3D_K_COUNT; ++i) {
        // reference = the 90th percentile of the launch durations: launches queued behind the convergence flag return at once (< 25 % of it),
        // and a launch that straddles a hiccup of the device (seen once: 19.9 ms for a 0.33 ms kernel) is not the kernel's duration either (> 4x)
        std::vector<float> sorted(c->timing.each[i]); std::sort(sorted.begin(), sorted.end());
        const float ref = sorted.empty() ? 0.0f : sorted[(size_t)(0.9 * (double)(sorted.size() - 1))];
        double s = 0.0, slow = 0.0; int64_t n = 0, nslow = 0;
        const bool waits_for_peers = i == I3D_K_COMM;        // exchange launches mostly WAIT: their spread is the peers', there is no "hiccup" to cut off
        for (float v : c->timing.each[i]) {
            if (v < 0.25f * ref) continue;
            if (v > 4.0f * ref && !waits_for_peers) { slow += v; ++nslow; continue; }
            s += v; ++n;
        }
        if (ms) ms[i] = s; if (launches) launches[i] = n;
        if (slow_ms) slow_ms[i] = slow; if (slow_launches) slow_launches[i] = nslow;      // reported beside the average, never silently dropped
    }
    return I3D_OK;
}
const char* i3d_kernel_name(int32_t k) {
    static const char* names[I3D_K_COUNT] = {"classify", "observe", "build", "eg_pass", "gather", "cost", "vector", "sh", "eg_aux", "comm", "eg_mr2", "eg_mr3"};
    return (k >= 0 && k < I3D_K_COUNT) ? names[k] : "?";
}
int i3d_problem_sizes(i3d_context* c, int64_t out[6]) { CTX_ENTER(c, out, I3D_ERR_INVALID_ARGUMENT); for (int i = 0; i < 6; ++i) out[i] = c->last_sizes[i]; return I3D_OK; }

void i3d_optimizer_config_default(i3d_optimizer_config* cfg) {     // optimizer.h:69-79, intrinsic3d.h:67-84
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->iterations = 10; cfg->lm_steps = 50; cfg->lambda_g = 0.2; cfg->lambda_r0 = 20.0; cfg->lambda_r1 = 160.0;
    cfg->lambda_s0 = 10.0; cfg->lambda_s1 = 120.0; cfg->lambda_a = 0.1;
    cfg->occlusion_distance = 0.02f; cfg->num_observations = 5; cfg->pcg_fixed_iterations = -1;
}

}  // extern "C"
