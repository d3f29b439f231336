// Host control of one Optimizer::optimize call on the device:
//   assemble()  = Optimizer::addVoxelResiduals over all voxels + NLSSolver::buildProblem (optimizer.cpp:119-165, nls_solver.cpp:190-276) — assemble.cpp
//   lm_solve()  = NLSSolver::solve (nls_solver.cpp:296-367): Ceres 2.1.0 TrustRegionMinimizer + LevenbergMarquardtStrategy + CGNR with
//                 block-Jacobi preconditioning [Ceres is un-vendored; semantics per SURVEY.md Appendix B], stopping after the first
//                 successful step (SuccessfulStepCallback, nls_solver.cpp:279-293); the CGNR solves themselves — pcg.cpp.
// Solver vectors are fp32 in work-list space; every reduction (dots, cost, weight sums, camera blocks) accumulates in fp64; the
// unknowns keep an fp64 master copy.  The PCG scalars stay on the device (PcgState); the host polls them one iteration behind.
#include "solver_internal.hpp"
#include <cstdlib>
#include <algorithm>

namespace i3d {

#ifdef I3D_MR_PHASES
void mr_phase_report_now();     // tile_pass_mr.hip, variant build only
#endif
#ifdef I3D_MR_BLOCKTIME
void mr_blocktime_report_now(); // tile_pass_mr.hip, variant build only
#endif

// The one place the solver's environment switches are read (SolverSwitches, context.hpp): at the top of every assemble and of estimate_sh.
void read_switches(i3d_context* c) {
    auto env = [](const char* name) { return std::getenv(name); };
    auto is = [&](const char* name, char v) { const char* e = env(name); return e && e[0] == v; };
    auto num = [&](const char* name, int unset) { const char* e = env(name); return e ? std::atoi(e) : unset; };
    auto clamp = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
    SolverSwitches w;
    { const char* e = env("I3D_DETERMINISTIC"); w.deterministic = e ? (e[0] == '1' ? 1 : 0) : -1; }      // 1 / 0: the bit-reproducible operator pass on / off (unset: on for one rank)
    w.ladder = clamp(num("I3D_LADDER", LADDER_MAX), 1, LADDER_MAX);      // LM attempts solved together; 1 = the serial trust-region loop
    w.ladder_mr = !is("I3D_LADDER_MR", '0');                             // 0: a ladder batch runs the single-system operator once per system (parity runs)
    w.ladder_mr1 = is("I3D_LADDER_MR1", '1');                            // 1: a lone live system of a batch goes through k_eg_tile_mr<1> as well
    w.ladder_group = clamp(num("I3D_LADDER_GROUP", 3), 1, 3);            // systems that share one stream of the rows
    w.ladder_pair = !is("I3D_LADDER_PAIR", '0');                         // 0: a pass of two groups is two launches instead of one paired launch
    w.egt_mr1 = is("I3D_EGT_MR1", '1');                                  // 1: the serial loop streams its rows through k_eg_tile_mr<1> (the control of the ladder tests)
    { const char* e = env("I3D_EGT_TILE"); w.egt_tile = e ? (std::atoi(e) == 512 ? 512 : 1024) : 0; }      // forces the tile geometry (unset: 1024, 512 on row-poor lists)
    w.hmax_limit = num("I3D_EGT_HMAX_LIMIT", 0);                         // tests of the overflow handling: halo slots the 512-entry geometry pretends to have
    w.hmax_limit_1024 = num("I3D_EGT_HMAX_LIMIT_1024", 0);               // ... and the 1024-entry geometry
    w.halo_pull = is("I3D_HALO_PULL", '1');                              // 1: halo sums pulled over plan lists outside the bit-reproducible mode too
    w.no_tile = is("I3D_NO_TILE", '1');                                  // 1: the untiled single-rank fallback (k_eg_jtjp + k_gather)
    { const char* e = env("I3D_NO_CULL"); w.no_cull = (e && e[0] >= '1' && e[0] <= '3') ? e[0] - '0' : 0; }      // 1 = no culling, 2 = no group masks, 3 = no weight-bound prefilter
    w.gradcol = !is("I3D_GRADCOL", '0');                                 // 0: gradient and column norms as two passes instead of one stream of the rows
    w.cost0 = !is("I3D_COST0", '0');                                     // 0: the initial cost from a residual-only pass instead of the assembly's sums
    w.debug_invalid_attempt = num("I3D_DEBUG_INVALID_ATTEMPT", -1);      // tests: this LM attempt's step counts as invalid
    { const int v = num("I3D_SH_SLAB", 0); w.sh_slab = v > 0 ? v : 0; }  // tests: chunks per launch of the SH Gram pass
    c->sw = w;
}

// wait for record `idx` of the current solve (mapped host memory, written by the LM kernels with a release store of its sequence number)
static int wait_record(i3d_context* c, int idx, int seq, LmRecord& out) {
    LmRecord* const r = c->h_lmrec + idx;
    const double t0 = now_s();
    while (__atomic_load_n(&r->seq, __ATOMIC_ACQUIRE) != seq) {
        if (now_s() - t0 > 60.0) {
            CTX_HIP(c, sync_stream(c));
            if (__atomic_load_n(&r->seq, __ATOMIC_ACQUIRE) != seq) return ctx_fail(c, I3D_ERR_HIP, "lm_solve: the device stopped publishing the state of the trust-region loop");
        }
    }
    out = *r;
    return I3D_OK;
}

// The route of this outer iteration's solves (the table at SolveRoute, solver_internal.hpp), decided once behind the assembly: the communicator is asked again
// here, after this iteration's shard_plan(), whatever plan_operator (assemble.cpp) heard before it.
static SolveRoute solve_route(i3d_context* c) {
    const int NS = 6 * c->K + 9;
    const bool sh = c->sharded();
    SolveRoute rt; std::memset(&rt.reduce_dev, 0, sizeof(rt.reduce_dev));
    rt.multi_system = multi_system_ok(c);
    // three launches per pass with the tiled operator; the six-launch sequence when untiled, or sharded with the exchanges as launches of the transport
    bool in_kernel = false;      // else, sharded: separate exchange launches (RCCL, or a rim that exceeds a mailbox)
    if (c->op.tile_ok && sh) { P2PDev probe; in_kernel = c->comm->fused_exchange(&probe) && NS + 2 <= probe.L.red_cap; }
    const bool three = c->op.tile_ok && (!sh || in_kernel);
    // the ladder: on one rank beside the three-launch pass; sharded with the exchanges as launches of the transport (the in-kernel mailbox exchanges keep the serial loop)
    bool ladder = c->op.ladder_max > 1 && c->op.tile_ok && (sh ? !in_kernel : true) && rt.multi_system;
    if (ladder && alloc_ladder(c) != I3D_OK) {      // (sharded: every rank holds the same list and takes the same decision unless its device alone is short of memory — then the collectives of the ranks no longer match and the run ends in the transport's time-out)
        ladder = false;
    }
    rt.loop = ladder ? PcgLoop::Ladder : (three ? PcgLoop::ThreeLaunch : PcgLoop::SixLaunch);
    rt.exchange = !sh ? Exchange::None : (three ? Exchange::InKernel : Exchange::Transport);
    if (sh && rt.loop == PcgLoop::SixLaunch) {      // the reductions of the six-launch pass inside its boundary kernels where the mailboxes are up and hold [camera block | p.q]
        const bool ok = c->comm->device_reduce(&rt.reduce_dev) && NS + 1 <= rt.reduce_dev.L.red_cap;
        if (ok) rt.exchange = Exchange::InKernelReduce; else rt.reduce_dev.on = 0;
    }
    return rt;
}

// NLSSolver::solve on the assembled rows.  Updates the device unknowns and the host camera when a step is accepted.
// The trust-region loop itself runs on the device (lm_kernels.hip); the host queues, per attempt,
//     k_lm_begin | PCG passes (polling the pass flags) | k_candidate | k_cand_frames | k_build<false> | k_lm_decide | k_accept
// and reads ONE record per attempt from mapped host memory — the record of attempt k-1 while the solve of attempt k is already queued (its kernels
// return at once when the loop has ended).  No stream synchronisation inside the loop; one at the end (accepted camera back to the host).
static int lm_solve(i3d_context* c, const i3d_optimizer_config& cfg, OptParams& p, i3d_iteration_stats* st, double initial_radius) {
    hipStream_t s = c->stream;
    const Layout L = layout_of(c);
    const int N = c->N, K = c->K, NP = (int)L.NP, NS = L.NS;
    GridView g = c->grid_view(); RowView r = c->row_view();
    LadderState& ld = c->ladder;
    if (cfg.lm_steps > LM_REC_SLOTS - 2) return ctx_fail(c, I3D_ERR_CAPACITY, "optimize: more than 62 LM steps per outer iteration");
    const SolveRoute route = solve_route(c);
    { TimedScope t(c, I3D_K_VECTOR); launch_freemask(s, r, p, c->v_mask.p); }
    // candidate arrays mirror x outside the work list (fixed parameters are read through them by the cost kernel)
    CTX_HIP(c, hipMemcpyAsync(c->xc_sdf.p, c->x_sdf.p, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(c->xc_alb.p, c->x_alb.p, sizeof(double) * (size_t)N, hipMemcpyDeviceToDevice, s));
    // column norms -> Jacobi scaling (computed once, TrustRegionMinimizer::Init); the camera blocks stay on the device for k_lm_begin
    // (one stream of the rows serves both on one rank: gradcol.hip; I3D_GRADCOL=0 keeps the two passes)
    const bool one_stream = one_stream_gradcol(c);
    auto after_colnorm = [&]() -> int {
        CTX_HIP(c, hipMemcpyAsync(c->d_cam_c.p, c->d_shared.p, sizeof(double) * (size_t)NS, hipMemcpyDeviceToDevice, s));
        CTX_HIP(c, hipMemcpyAsync(c->d_cam_H.p, c->d_blocks.p, sizeof(double) * ((size_t)21 * K + 25), hipMemcpyDeviceToDevice, s));
        { int rc2 = allgather(c, c->v_c.p); if (rc2) return rc2; }     // the candidate point needs S everywhere
        { TimedScope t(c, I3D_K_VECTOR); launch_scale_from_colnorm(s, NP, c->v_c.p, c->v_mask.p, c->v_S.p, c->v_cm.p); }
        return I3D_OK;
    };
    int rc = I3D_OK;
    if (one_stream) { rc = run_gradcol(c, p, after_colnorm); if (rc) return rc; }
    else {
        rc = run_pass(c, PASS_COLNORM, p, nullptr, c->v_c.p); if (rc) return rc;
        rc = after_colnorm(); if (rc) return rc;
        // gradient b = S J^T W r and initial cost
        rc = run_pass(c, PASS_GRAD, p, nullptr, c->v_acc.p); if (rc) return rc;
    }
    { TimedScope t(c, I3D_K_VECTOR); launch_mul(s, NP, c->v_S.p, c->v_acc.p, c->v_b.p); }
    // initial cost -> d_scal[16]: from the residuals the assembly already holds (I3D_COST0=0: the residual-only pass at the unchanged point, as up to round 4)
    if (!c->sw.cost0) { rc = eval_cost_launch(c, p, false, c->d_frames.p); if (rc) return rc; }
    else if (!one_stream) { TimedScope t(c, I3D_K_VECTOR); launch_set_double(s, c->d_scal.p + 16, c->cost_at_build); }      // (one stream: k_eg_gradcol left it there)
    rc = count_above_dev(c, c->v_acc.p, c->v_mask.p, 1e-10f, c->d_scal.p + 8); if (rc) return rc;   // gradient_tolerance: free entries of g = J^T W r above 1e-10 (max-norm test)
    rc = dot_dev(c, c->v_mask.p, c->v_mask.p, c->d_scal.p + 9); if (rc) return rc;           // free parameters
    {   // camera unknowns of the current point for the candidate kernel (staged in pinned memory: the copy is asynchronous)
        double* xs = c->h_pinned;
        for (int i = 0; i < 6 * K; ++i) xs[i] = c->poses[i];
        for (int i = 0; i < 4; ++i) xs[6 * K + i] = c->intr[i];
        for (int i = 0; i < 5; ++i) xs[6 * K + 4 + i] = c->dist[i];
        CTX_HIP(c, hipMemcpyAsync(c->d_xshared.p, xs, sizeof(double) * NS, hipMemcpyHostToDevice, s));
    }
    const int seq0 = c->lm_seq; c->lm_seq += LM_REC_SLOTS;
    LmState* const lm = c->d_lm.p;
    launch_lm_init(s, lm, c->d_scal.p + 16, c->d_scal.p + 8, c->d_scal.p + 9, initial_radius, c->d_lmrec, seq0);

    int attempts = 0; bool ended = false, accepted = false;
    // one record consumed: statistics + whether the solve is over
    auto consume = [&](const LmRecord& rec) {
        if (rec.kind == 0) {
            if (st) { st->cost_initial = rec.cost; st->cost_final = rec.cost; st->free_parameters = (int64_t)(rec.nfree + 0.5); st->termination = rec.final_ ? 1 : 0; st->final_radius = initial_radius; }
            c->last_sizes[5] = (long long)(rec.nfree + 0.5);
        } else if (rec.kind == 2) { if (st) st->termination = 1; }                            // the radius ran out before the attempt (LevenbergMarquardtStrategy)
        else {
            if (st) {
                st->lm_iterations = attempts + 1;
                if (attempts < 50) { st->pcg_iterations[attempts] = rec.pcg_it; st->step_accepted[attempts] = rec.accepted; }
                st->final_radius = rec.radius_after; st->termination = rec.termination;
                if (rec.accepted) { st->cost_final = rec.cost; st->successful_steps += 1; }
            }
            if (cfg.verbose) std::printf("  [i3d LM] it %d cand %.9e model %.3e rho %.4f radius -> %.3e cg %d%s\n", attempts + 1, rec.cand_cost, rec.model_change, rec.rel, rec.radius_after, rec.pcg_it,
                                         rec.accepted ? " accepted" : "");
            accepted = rec.accepted != 0;
            ++attempts;
        }
        if (rec.final_) ended = true;
    };
    // The decision chain of one attempt, all on the stream: the candidate point of the step `x` (replicated: every rank holds the whole step), its keyframe constants and
    // its cost, then k_lm_decide on the terminal PCG state `ps` and k_accept.  lad_next: the position behind this attempt in its ladder batch (serial loop: -1).
    auto queue_decision = [&](const float* x, const PcgState* ps, int attempt, int lad_next) -> int {
        { TimedScope t(c, I3D_K_VECTOR);
          launch_candidate(s, g, r, K, -1.0f, x, c->v_S.p, c->d_xshared.p, c->xc_sdf.p, c->xc_alb.p, c->d_xcshared.p, c->d_scal.p + 4, c->v_mask.p, c->d_partials.p, lm);
          launch_cand_frames(s, K, c->d_xcshared.p, c->d_frames.p, c->d_frames_cand.p, lm); }
        const int rc2 = eval_cost_launch(c, p, true, c->d_frames_cand.p, c->d_xcshared.p + 6 * K, lm); if (rc2) return rc2;
        { TimedScope t(c, I3D_K_VECTOR);
          launch_lm_decide(s, lm, ps, c->d_scal.p + 4, c->d_scal.p + 16, attempt, cfg.lm_steps, c->d_lmrec + 1 + attempt, seq0 + 1 + attempt, lad_next,
                           c->sw.debug_invalid_attempt == attempt ? 1 : 0);      // (I3D_DEBUG_INVALID_ATTEMPT: this attempt's step counts as invalid)
          launch_accept(s, g, r, c->xc_sdf.p, c->xc_alb.p, lm); }
        return I3D_OK;
    };
    // The damping ladder: batches of consecutive attempts are SOLVED together (k_lm_begin_lad: the radii a run of rejections leads to; pcg_solve_ladder: lock step, the
    // rows streamed once per group of systems) and then DECIDED one after the other by the same k_lm_decide — results, attempts, accept sequence and PCG counts are
    // those of the serial loop (bit for bit in the bit-reproducible mode).  Batch depth: what the previous outer iteration needed (the reference restarts at radius 1e4
    // every time, optimizer.cpp:138, so the count barely moves), doubling while everything is rejected.  An invalid step (radius halved instead of divided) puts a
    // batch out of step: the attempt behind it is solved again on its own (LmRecord kind 3).
    if (route.loop == PcgLoop::Ladder) {
        const LadVec& lv = ld.strides;
        { LmRecord rec; rc = wait_record(c, 0, seq0, rec); if (rc) return rc; consume(rec); }      // the initial tests
        // Batch depth.  First batch: what the last two outer iterations needed (the larger: one system too many costs its few PCG passes at the marginal price of a
        // shared stream, one too few costs a second batch); without history 2, doubling while everything is rejected.  With history, a batch that ends without an
        // accepted step is followed by batches of 2: the accepting attempt is near (a second full-depth batch wasted 5 of its 6 systems, profiles/r05_ladder_policy.json).
        const bool warm = ld.hint > 0;
        int k = 0, prevB = 0; bool after_resync = false;
        while (k < cfg.lm_steps && !ended) {
            int B = after_resync ? 1 : (prevB == 0 ? (warm ? std::max(ld.hint, ld.hint_prev) : 2) : (warm ? 2 : 2 * prevB));
            B = std::max(1, std::min(B, std::min(c->op.ladder_max, cfg.lm_steps - k)));
            after_resync = false; prevB = B;
            { TimedScope t(c, I3D_K_VECTOR);
              launch_lm_begin_lad(s, lm, B, K, p.fix_poses, p.fix_intr, p.fix_dist, c->d_cam_c.p, c->d_cam_H.p, ld.mblk.p, lv.mblk, c->v_c.p + L.tail_off, c->v_S.p + L.tail_off, ld.tail.p, lv.tail,
                                  c->d_lmrec + 1 + k, seq0 + 1 + k); }
            const PcgState* fin[LADDER_MAX] = {nullptr};
            rc = pcg_solve_ladder(c, route, cfg, p, B, fin); if (rc) return rc;
            ++ld.batches;
            for (int j = 0; j < B && c->sharded(); ++j) { rc = allgather(c, lad_vecp(c, LV_X, j)); if (rc) return rc; }      // the candidate points are replicated: every rank needs the whole step of every system
            // the decision chain of every system, in ladder order; everything behind the deciding attempt returns at once
            for (int j = 0; j < B; ++j) { rc = queue_decision(lad_vecp(c, LV_X, j), fin[j], k + j, j + 1); if (rc) return rc; }
            int decided = 0;
            for (int j = 0; j < B && !ended; ++j) {
                LmRecord rec; rc = wait_record(c, 1 + k + j, seq0 + 1 + k + j, rec); if (rc) return rc;
                if (rec.kind == 3) {            // out of step: attempt k + j was solved with a radius the trust region did not reach — solve it again, alone
                    __atomic_store_n(&c->h_lmrec[1 + k + j].seq, 0, __ATOMIC_RELEASE);
                    ++ld.resyncs; after_resync = true; break;
                }
                consume(rec); ++decided;
            }
            if (ended && decided < B) ld.wasted += B - decided;
            k += decided;
        }
        if (attempts > 0) { ld.hint_prev = ld.hint; ld.hint = attempts; }
        ended = true;        // (every record of the solve has been consumed)
    }
    const bool three = route.loop == PcgLoop::ThreeLaunch;
    int k = 0;
    for (; route.loop != PcgLoop::Ladder && k < cfg.lm_steps; ++k) {
        // attempt k, queued behind whatever attempt k-1 still has in flight.  k_lm_begin: radius test, 1/radius, LM diagonal of the camera tail, block-Jacobi
        // inverses of the damped camera blocks
        { TimedScope t(c, I3D_K_VECTOR);
          launch_lm_begin(s, lm, K, p.fix_poses, p.fix_intr, p.fix_dist, c->d_cam_c.p, c->d_cam_H.p, c->Minv_blocks.p, c->v_c.p + L.tail_off, c->v_S.p + L.tail_off, c->v_D2.p + L.tail_off, c->v_Minv.p + L.tail_off,
                          c->d_lmrec + 1 + k, seq0 + 1 + k);
          if (!three) launch_lm_diag_dev(s, (int)L.tail_off, c->v_c.p, c->v_S.p, lm, c->v_D2.p, c->v_Minv.p); }      // (the three-launch pass recomputes S, D^2, M^-1 of the voxel unknowns from the column norms)
        const PcgState* ps = nullptr;
        // (one rank reaches the six-launch loop only untiled: tile_ok routes it to the three-launch pass, so pcg_solve has no single-rank tiled arm)
        rc = three ? pcg_solve_fused(c, route, cfg, p, &ps) : pcg_solve(c, route, cfg, p, &ps); if (rc) return rc;
        // the pass flags this solve waited for were written after everything queued before it: record k (initial tests for k = 0, else attempt k-1) is there
        { LmRecord rec; rc = wait_record(c, k, seq0 + k, rec); if (rc) return rc; consume(rec); }
        if (ended) break;
        // candidate point (replicated: every rank needs the whole step), its keyframe constants and its cost, then the decision — all on the stream
        { int rc2 = allgather(c, c->v_x.p); if (rc2) return rc2; }
        rc = queue_decision(c->v_x.p, ps, k, -1); if (rc) return rc;
    }
    if (!ended) { LmRecord rec; rc = wait_record(c, k, seq0 + k, rec); if (rc) return rc; consume(rec); }      // the last attempt's record (step limit)
    if (st) st->num_attempts = std::min(attempts, 50);
    // the accepted camera back to the host (the next outer iteration rebuilds its keyframe constants from it)
    CTX_HIP(c, hipMemcpyAsync(c->h_pinned, c->d_xcshared.p, sizeof(double) * NS, hipMemcpyDeviceToHost, s));
    CTX_HIP(c, sync_stream(c));
    if (c->sharded() && c->comm->health(s)) return ctx_fail(c, I3D_ERR_COMM, "lm_solve: a peer-to-peer exchange timed out (a rank stopped taking part)");
    if (accepted) {
        for (int i = 0; i < 6 * K; ++i) c->poses[i] = c->h_pinned[i];
        for (int i = 0; i < 4; ++i) c->intr[i] = c->h_pinned[6 * K + i];
        for (int i = 0; i < 5; ++i) c->dist[i] = c->h_pinned[6 * K + 4 + i];
    }
    { const int lrc = ctx_launch_check(c); if (lrc) return lrc; }
    return I3D_OK;
}

int optimize(i3d_context* c, const i3d_optimizer_config& cfg, i3d_iteration_stats* stats) {
    if (!c->have_grid || cfg.iterations < 1) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "optimize: no grid or iterations < 1");   // optimizer.cpp:113-114
    CTX_HIP(c, hipSetDevice(c->device));
    double carried_radius = 1e4;
    for (int itr = 0; itr < cfg.iterations; ++itr) {
        i3d_iteration_stats local; std::memset(&local, 0, sizeof(local));
        i3d_iteration_stats* st = stats ? &stats[itr] : &local;
        std::memset(st, 0, sizeof(*st));
        OptParams p;
        const double t0 = now_s();
        int rc = assemble(c, cfg, itr, p, st); if (rc) return rc;
        const double t1 = now_s();
        // t_add_end: device time from the start of the assembly to the end of the residual collection (events on the stream)
        st->time_add = (c->t_add_end >= 0.0 && c->t_add_end <= t1 - t0) ? c->t_add_end : t1 - t0; st->time_build = (t1 - t0) - st->time_add;
        if (c->n_active > 0) { rc = lm_solve(c, cfg, p, st, cfg.carry_trust_radius ? carried_radius : 1e4); if (rc) return rc;
                               if (st->final_radius > 0.0) carried_radius = st->final_radius; }
        const double t2 = now_s();
        st->time_solve = t2 - t1;
        if (cfg.verbose) std::printf("[i3d] itr %d rows %lld/%lld/%lld/%lld valid %lld cost %.9e -> %.9e (add %.3f ms, solve %.3f ms)\n", itr,
                                     (long long)st->rows[0], (long long)st->rows[1], (long long)st->rows[2], (long long)st->rows[3], (long long)st->valid_voxels,
                                     st->cost_initial, st->cost_final, st->time_add * 1e3, st->time_solve * 1e3);
        timing_flush(c);
    }
    c->assembled = false;
#ifdef I3D_MR_PHASES
    mr_phase_report_now();      // (variant build only: tools/build_variant.sh)
#endif
#ifdef I3D_MR_BLOCKTIME
    mr_blocktime_report_now();
#endif
    return I3D_OK;
}

}  // namespace i3d
