// extern "C" entry points around the solve: optimize, the one-shot host drop-in, the communicator and its host statements, i3d_debug_assemble and the solver's
// counters.  (The readbacks of assembled solver state: solver_debug.cpp.)
#include <cstdlib>
#include "context.hpp"

using namespace i3d;

extern "C" {

int i3d_optimize(i3d_context* c, const i3d_optimizer_config* cfg, i3d_iteration_stats* stats) {
    CTX_ENTER(c, cfg, ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_optimize: null argument"));
    return optimize(c, *cfg, stats);
}

int i3d_optimize_host(int32_t device_ordinal, const i3d_optimizer_config* cfg, const i3d_grid_view* grid,
                      double* sdf_refined_io, double* albedo_io, int32_t num_frames, int32_t levels, const int32_t* widths,
                      const int32_t* heights, const float* const* lum, const float* const* depth,
                      double* intr_io, double* dist_io, double* poses_io, const double* voxel_sh, i3d_iteration_stats* stats) {
    if (!cfg || !grid || !sdf_refined_io || !albedo_io || !intr_io || !dist_io || !poses_io || !voxel_sh) return I3D_ERR_INVALID_ARGUMENT;
    i3d_context* c = nullptr;
    int rc = i3d_create(device_ordinal, &c); if (rc) return rc;
    i3d_grid_view gv = *grid; gv.sdf_refined = sdf_refined_io; gv.albedo = albedo_io;
    rc = i3d_set_grid(c, &gv);
    if (!rc) rc = i3d_set_frames(c, num_frames, levels, widths, heights, lum, depth, nullptr);
    if (!rc) rc = i3d_set_camera(c, intr_io, dist_io, poses_io);
    if (!rc) rc = i3d_set_voxel_sh(c, voxel_sh);
    if (!rc) rc = i3d_optimize(c, cfg, stats);
    if (!rc) rc = i3d_get_grid(c, sdf_refined_io, albedo_io);
    if (!rc) rc = i3d_get_camera(c, intr_io, dist_io, poses_io);
    if (rc) std::fprintf(stderr, "i3d_optimize_host: %s\n", i3d_last_error(c));
    i3d_destroy(c);
    return rc;
}

int i3d_comm_unique_id(void* out128, int32_t* bytes) {
    if (!out128 || !bytes) return I3D_ERR_INVALID_ARGUMENT;
    size_t n = 0; if (rccl_unique_id(out128, &n)) return I3D_ERR_COMM;
    *bytes = (int32_t)n; return I3D_OK;
}
int i3d_comm_init(i3d_context* c, int32_t rank, int32_t world, const void* unique_id, int32_t id_bytes) {
    CTX_ENTER(c, unique_id && world >= 1 && rank >= 0 && rank < world, ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_comm_init: bad arguments"));
    char err[256] = {0};
    Comm* cm = make_rccl_comm(rank, world, unique_id, (size_t)id_bytes, c->stream, err, sizeof(err));
    if (!cm) return ctx_fail(c, I3D_ERR_COMM, err);
    { const char* e = std::getenv("I3D_FORCE_COLLECTIVES"); cm->force = e && e[0] == '1'; }      // test hook: sharded path with a 1-rank communicator
    delete c->comm; c->comm = cm; c->assembled = false; c->slots = 0;      // solver vectors are sized for the world: re-derive storage
    return I3D_OK;
}
void* i3d_comm_sim_create(int32_t world) { return world >= 1 ? sim_create(world) : nullptr; }
void i3d_comm_sim_destroy(void* shared) { if (shared) sim_destroy((SimShared*)shared); }
int i3d_comm_init_sim(i3d_context* c, void* shared, int32_t rank) {
    CTX_ENTER(c, shared, ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_comm_init_sim: bad arguments"));
    delete c->comm; c->comm = make_sim_comm((SimShared*)shared, rank); c->assembled = false; c->slots = 0;
    return I3D_OK;
}

int i3d_shard_plan(int32_t A, int32_t world, int32_t rank, const int32_t* anbr, const uint8_t* active, int32_t* chunk, int32_t* own0,
                   int32_t* own1, uint8_t* in_compute_list) {
    if (A < 0 || world < 1 || rank < 0 || rank >= world || !chunk || !own0 || !own1) return I3D_ERR_INVALID_ARGUMENT;
    int ch, o0, o1; shard_range(A, world, rank, ch, o0, o1);
    *chunk = ch; *own0 = o0; *own1 = o1;
    if (in_compute_list && anbr && active)
        for (int a = 0; a < A; ++a) in_compute_list[a] = shard_needs_entry(a, o0, o1, active[a] != 0, anbr, (size_t)A) ? 1 : 0;
    return I3D_OK;
}
int32_t i3d_shard_vec_index(int32_t a, int32_t chunk, int32_t albedo) { return albedo ? vec_alb(a, chunk) : vec_sdf(a, chunk); }
// need[e] bit k: rank k's rows read the unknowns of entry e and it does not own e — the host statement of k_need_mask (shard_kernels.hip)
int i3d_shard_need(int32_t A, int32_t world, const int32_t* anbr, const uint8_t* active, uint64_t* need) {
    if (A < 0 || world < 1 || world > 64 || !anbr || !active || !need) return I3D_ERR_INVALID_ARGUMENT;
    int chunk, o0, o1; shard_range(A, world, 0, chunk, o0, o1);
    const int slice = chunk / world;
    for (int a = 0; a < A; ++a) need[a] = 0;
    for (int a = 0; a < A; ++a) {
        if (!active[a]) continue;
        int col[12]; bool interior;
        const unsigned long long ranks = shard_entry_ranks(a, slice, anbr, (size_t)A, col, interior);
        if (interior) continue;
        for (int k = 0; k < world; ++k) if ((ranks >> k) & 1ull) {
            if (a / slice != k) need[a] |= 1ull << k;
            for (int i = 0; i < 12; ++i) if (col[i] >= 0 && col[i] / slice != k) need[col[i]] |= 1ull << k;
        }
    }
    return I3D_OK;
}
int i3d_comm_stats(i3d_context* c, int64_t* halo_calls, int64_t* halo_bytes_sent, int64_t* reduce_calls, int64_t* reduce_bytes, int32_t* halo_entries_send, int32_t* halo_entries_recv,
                   int32_t* ghost_tiles, int32_t* compute_list) {
    CTX_ENTER(c, true, I3D_ERR_INVALID_ARGUMENT);
    if (halo_calls) *halo_calls = c->comm ? c->comm->halo_calls : 0; if (halo_bytes_sent) *halo_bytes_sent = c->comm ? c->comm->halo_bytes_sent : 0;
    if (reduce_calls) *reduce_calls = c->comm ? c->comm->reduce_calls : 0; if (reduce_bytes) *reduce_bytes = c->comm ? c->comm->reduce_bytes : 0;
    if (halo_entries_send) *halo_entries_send = c->shard.halo.n_send; if (halo_entries_recv) *halo_entries_recv = c->shard.halo.n_recv;
    if (ghost_tiles) *ghost_tiles = c->shard.n_ghost_tiles; if (compute_list) *compute_list = c->shard.nC;
    return I3D_OK;
}

const char* i3d_comm_transport(i3d_context* c) { return (c && c->comm) ? c->comm->transport : ""; }

int i3d_debug_assemble(i3d_context* c, const i3d_optimizer_config* cfg, int32_t iteration, int32_t* slots_out) {
    CTX_ENTER(c, cfg, ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_debug_assemble: null argument"));
    OptParams p; i3d_iteration_stats st; std::memset(&st, 0, sizeof(st));
    int rc = assemble(c, *cfg, iteration, p, &st);
    if (!rc && slots_out) *slots_out = c->slots;
    return rc;
}

int i3d_debug_counters(i3d_context* c, int64_t* stream_syncs) {
    CTX_ENTER(c, true, I3D_ERR_INVALID_ARGUMENT);
    if (stream_syncs) *stream_syncs = (int64_t)c->n_syncs;
    return I3D_OK;
}

int i3d_debug_ladder_stats(i3d_context* c, int64_t* out6) {
    CTX_ENTER(c, out6, I3D_ERR_INVALID_ARGUMENT);
    out6[0] = c->ladder.batches; out6[1] = c->ladder.streams; out6[2] = c->ladder.system_passes; out6[3] = c->ladder.resyncs; out6[4] = c->ladder.wasted; out6[5] = c->op.ladder_max;
    return I3D_OK;
}
int i3d_debug_ladder_passes(i3d_context* c, int64_t* out8) {
    CTX_ENTER(c, out8, I3D_ERR_INVALID_ARGUMENT);
    for (int n = 0; n < 7; ++n) out8[n] = c->ladder.pass_live[n];
    out8[7] = c->ladder.paired;
    return I3D_OK;
}

}  // extern "C"
