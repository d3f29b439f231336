// What the translation units of the solver host share (solver.cpp: the switches, the trust-region loop, optimize; assemble.cpp: the work list, the sharding plan,
// the operator plan; pcg.cpp: the normal-equation passes and the three PCG drivers; solver_debug.cpp: the parity probes): the vector layout, the strides of the
// partial-row buffers, the collectives of a sharded run, the counted synchronisation and the route of a solve.
#pragma once
#include "context.hpp"
#include <chrono>
#include <functional>

namespace i3d {

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

constexpr int AUX_PART_ROWS = 320;     // >= the workgroups of a gradient / column-norm pass (one per CU)
inline size_t aux_part_stride(int K) { return ((size_t)21 * K + 34 + 3) & ~(size_t)3; }
constexpr int GC_PART_ROWS = 1024;     // >= the workgroups of the one-stream gradient + column-norm pass (two per CU)
inline size_t gc_col_off(int K) { return ((size_t)6 * K + 9 + 3) & ~(size_t)3; }
inline size_t gc_part_stride(int K) { return gc_col_off(K) + aux_part_stride(K); }
constexpr int LM_REC_SLOTS = 64;       // LmRecord ring: the initial tests + one record per LM attempt (lm_steps <= LM_REC_SLOTS - 2)

// every stream synchronisation of the solver path goes through here (counted: i3d_debug_counters; the review bar is <= 8 per Gauss-Newton iteration)
inline hipError_t sync_stream(i3d_context* c) { ++c->n_syncs; return hipStreamSynchronize(c->stream); }

// vector layout (common.hpp): [sdf chunk | albedo chunk | camera tail]; a rank's slice = the same segment of both parts
struct Layout { int A, K, NS, chunk, world, rank, slice; Seg2 own; size_t tail_off, NP; };
inline Layout layout_of(const i3d_context* c) {
    Layout L; L.A = c->A; L.K = c->K; L.NS = 6 * c->K + 9; L.chunk = c->shard.chunk; L.world = c->comm ? c->comm->world : 1; L.rank = c->comm ? c->comm->rank : 0;
    L.slice = L.chunk / L.world;
    L.own = Seg2{(size_t)L.rank * L.slice, (size_t)L.chunk + (size_t)L.rank * L.slice, L.slice};
    L.tail_off = 2 * (size_t)L.chunk; L.NP = L.tail_off + L.NS;
    return L;
}
// Where the cost the trust-region loop starts from comes from (it is the cost at the point the rows were built at; up to round 4: a residual-only pass k_build<false>):
//   one rank           : the gradient pass (gradcol.hip) adds up 0.5 w r^2 of the rows it streams anyway;
//   sharded / I3D_GRADCOL=0 : k_weight_sums adds the per-type sums while it walks the row weights (assemble);
//   I3D_COST0=0        : the residual-only pass.
inline bool one_stream_gradcol(const i3d_context* c) { return !c->sharded() && c->sw.gradcol; }
inline bool cost_from_sums(const i3d_context* c) { return c->sw.cost0 && !one_stream_gradcol(c); }

inline int allreduce(i3d_context* c, double* dev, size_t n) {
    if (!c->sharded()) return I3D_OK;
    TimedScope t(c, I3D_K_COMM);
    return c->comm->allreduce_sum(dev, n, c->stream) ? ctx_fail(c, I3D_ERR_COMM, "all-reduce failed") : I3D_OK;
}
inline int allgather(i3d_context* c, float* vec) {       // every rank contributes its two segments of a solver vector
    if (!c->sharded()) return I3D_OK;
    const size_t slice = (size_t)(c->shard.chunk / c->comm->world);
    TimedScope t(c, I3D_K_COMM);
    if (c->comm->allgather(vec, slice, c->stream) || c->comm->allgather(vec + c->shard.chunk, slice, c->stream)) return ctx_fail(c, I3D_ERR_COMM, "all-gather failed");
    return I3D_OK;
}
inline int push_halo(i3d_context* c, float* vec) {       // the rim of the operator input (common.hpp: sharding)
    if (!c->sharded()) return I3D_OK;
    TimedScope t(c, I3D_K_COMM);
    return c->comm->push_halo(vec, c->shard.halo, c->stream) ? ctx_fail(c, I3D_ERR_COMM, "halo exchange failed") : I3D_OK;
}

// read `n` doubles from device memory (after everything queued on the stream)
inline int read_doubles(i3d_context* c, const double* dptr, size_t n, double* out) {
    CTX_HIP(c, hipMemcpyAsync(c->h_pinned, dptr, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    CTX_HIP(c, sync_stream(c));
    std::memcpy(out, c->h_pinned, n * sizeof(double));
    return I3D_OK;
}

// The multi-system operator pass (tile_pass_mr.hip) can run on the current plan: it exists in the 512-entry geometry, reads its halo over the pull lists and is
// built for the shipped 5 observation slots.
inline bool multi_system_ok(const i3d_context* c) { return c->plan_T() == 512 && c->tile_plan().hp_off != nullptr && c->slots == 5; }

// Which solve an outer iteration's LM attempts run, decided once at the top of lm_solve (solve_route, solver.cpp) and handed to the drivers of pcg.cpp:
//   operator          ranks    transport of the exchanges          loop          exchange
//   untiled           1        -                                   SixLaunch     None
//   tiled             1        -                                   Ladder *      None
//   tiled             > 1 **   mailboxes, every rim fits           ThreeLaunch   InKernel
//   tiled             > 1      launches (RCCL, rank simulation)    Ladder *      Transport
//   tiled             > 1      mailboxes, a rim does not fit ***   Ladder *      Transport; the SixLaunch fall-back: InKernelReduce
// *   where the ladder cannot run (I3D_LADDER=1, the multi-system pass not available, its slabs do not fit the device): ThreeLaunch on one rank, SixLaunch sharded
// **  or one rank forced onto the sharded path (I3D_FORCE_COLLECTIVES)
// *** or the camera block + 2 doubles exceed the mailbox's reduction slots
enum class PcgLoop { SixLaunch, ThreeLaunch, Ladder };      // pcg_solve | pcg_solve_fused | pcg_solve_ladder
enum class Exchange {
    None,               // one rank
    Transport,          // every reduction and rim exchange of a pass is a launch of the transport
    InKernelReduce,     // the reductions run inside the boundary kernels (k_pcg_tail_a / k_pcg_tail_b), the rim is pushed by a launch of the transport
    InKernel            // reductions and rim inside the PCG kernels (pcg_fused.hip)
};
struct SolveRoute {
    PcgLoop loop = PcgLoop::SixLaunch; Exchange exchange = Exchange::None;
    bool multi_system = false;      // multi_system_ok at the time of the decision
    P2PDev reduce_dev;              // InKernelReduce: the mailboxes as the boundary kernels take them
};

// pcg.cpp — the normal-equation passes (GRAD / COLNORM / JTJP -> out[NP]) and what the trust-region loop queues around the solves
int run_pass(i3d_context* c, PassMode mode, const OptParams& p, const float* u, float* out);
int run_gradcol(i3d_context* c, const OptParams& p, const std::function<int()>& between);
int dot_dev(i3d_context* c, const float* a, const float* b, double* slot);
int count_above_dev(i3d_context* c, const float* a, const float* m, float tol, double* slot);
int eval_cost_launch(i3d_context* c, const OptParams& p, bool candidate, const FrameConst* frames, const double* cam9 = nullptr, const LmState* lm = nullptr);
// the slabs of a ladder batch (non-zero WITHOUT a latched error: they do not fit the device) and a system's vector of one kind in them
int alloc_ladder(i3d_context* c);
enum { LV_X = 0, LV_R, LV_P, LV_Z, LV_U, LV_Q };
inline float* lad_vecp(const i3d_context* c, int kind, int sys = 0) { return c->ladder.vec.p + ((size_t)kind * c->op.ladder_max + sys) * c->ladder.strides.vec; }
// the three drivers: one system (*final_state: its terminal state on the device) in six or three launches per pass, or the B systems of a ladder batch in lock step
int pcg_solve(i3d_context* c, const SolveRoute& route, const i3d_optimizer_config& cfg, const OptParams& p, const PcgState** final_state);
int pcg_solve_fused(i3d_context* c, const SolveRoute& route, const i3d_optimizer_config& cfg, const OptParams& p, const PcgState** final_state);
int pcg_solve_ladder(i3d_context* c, const SolveRoute& route, const i3d_optimizer_config& cfg, const OptParams& p, int B, const PcgState** finals);

}  // namespace i3d
