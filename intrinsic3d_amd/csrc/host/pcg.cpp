// The normal-equation passes and the PCG solves of the trust-region loop (lm_solve, solver.cpp): CGNR with block-Jacobi preconditioning [Ceres 2.1.0
// ConjugateGradientsSolver; semantics per SURVEY.md Appendix B] in three drivers that share one pass protocol — six launches per pass, three launches per pass, and
// the lock-step solve of a ladder batch.  Solver vectors are fp32 in work-list space; every reduction (dots, cost, weight sums, camera blocks) accumulates in fp64.
// The PCG scalars stay on the device (PcgState); the host polls them through a ring of pass numbers in mapped memory.
#include "solver_internal.hpp"
#include <algorithm>

namespace i3d {

// ---- normal-equation pieces (GRAD / COLNORM; the PCG operator is inlined in the drivers) ------------------------------------------------------------
int run_pass(i3d_context* c, PassMode mode, const OptParams& p, const float* u, float* out /*[NP]*/) {
    hipStream_t s = c->stream; GridView g = c->grid_view(); RowView r = c->row_view(); const Layout L = layout_of(c);
    const int stride = (int)aux_part_stride(c->K);
    PassBuffers b{c->C.p, c->treg.p, c->d_shared.p, c->d_blocks.p, c->aux_part.p, stride};
    CTX_HIP(c, hipMemsetAsync(c->d_shared.p, 0, sizeof(double) * ((size_t)L.NS + 1), s));
    if (mode == PASS_COLNORM) CTX_HIP(c, hipMemsetAsync(c->d_blocks.p, 0, sizeof(double) * (21 * (size_t)c->K + 25), s));
    // the camera block leaves every launch as one float row per workgroup, added up in workgroup order (launch_sum_rows): no global atomics, bit-reproducible
    if (mode == PASS_JTJP && c->op.tile_ok && !c->sharded()) {        // the PCG's tiled operator pass (raw accumulators straight into `out`)
        const int NSP = (L.NS + 3) & ~3; int rows = 0;
        { TimedScope t(c, I3D_K_EG_PASS); rows = launch_eg_tile(s, r, p, u, c->tile_plan(), nullptr, out, nullptr, nullptr, c->cam_part.p, NSP); }
        { TimedScope t(c, I3D_K_GATHER); launch_halo_fold(s, r, c->tile_plan(), out, nullptr); }
        { TimedScope t(c, I3D_K_VECTOR); launch_mul(s, 2 * c->shard.chunk, c->v_mask.p, out, out);       // the raw accumulators also cover fixed unknowns (the PCG multiplies them by S = 0)
          if (rows > 0) launch_sum_rows(s, PASS_JTJP, c->K, c->cam_part.p, rows, NSP, c->d_shared.p, c->d_blocks.p); }
    } else {
        int rows = 0;
        { TimedScope t(c, mode == PASS_JTJP ? I3D_K_EG_PASS : I3D_K_EG_AUX); rows = launch_eg_pass(s, mode, g, r, p, u, b, nullptr);
          if (rows > AUX_PART_ROWS) return ctx_fail(c, I3D_ERR_CAPACITY, "run_pass: more workgroups than rows of the camera partial buffer");
          if (rows > 0) launch_sum_rows(s, mode, c->K, c->aux_part.p, rows, stride, c->d_shared.p, c->d_blocks.p); }
        { TimedScope t(c, I3D_K_GATHER); launch_gather(s, mode, r, b, out); }
    }
    { int rc = allreduce(c, c->d_shared.p, (size_t)L.NS); if (rc) return rc; }
    if (mode == PASS_COLNORM) { int rc = allreduce(c, c->d_blocks.p, 21 * (size_t)c->K + 25); if (rc) return rc; }
    { TimedScope t(c, I3D_K_VECTOR); launch_shared_finalize(s, L.tail_off, c->K, p, c->d_shared.p, out, false, nullptr, nullptr, nullptr, nullptr, nullptr); }
    return I3D_OK;
}

// Column norms -> c->v_c (+ d_shared / d_blocks: the camera part and the camera blocks) and the raw gradient J^T W r -> c->v_acc from ONE stream of the rows
// (gradcol.hip).  One rank only (a sharded run keeps the two passes: their all-reduces sit between the launches).  `between` runs after the column norms are
// complete and before d_shared is reused for the gradient's camera part.
int run_gradcol(i3d_context* c, const OptParams& p, const std::function<int()>& between) {
    hipStream_t s = c->stream; GridView g = c->grid_view(); RowView r = c->row_view(); const Layout L = layout_of(c);
    const int stride = (int)gc_part_stride(c->K), col_off = (int)gc_col_off(c->K);
    GradColBuffers gb{c->C.p, c->C2.p, c->treg.p, c->treg2.p, c->gc_part.p, stride, col_off, c->d_partials.p, c->d_scal.p + 16};
    CTX_HIP(c, hipMemsetAsync(c->d_scal.p + 16, 0, sizeof(double), s));
    CTX_HIP(c, hipMemsetAsync(c->d_shared.p, 0, sizeof(double) * ((size_t)L.NS + 1), s));
    CTX_HIP(c, hipMemsetAsync(c->d_blocks.p, 0, sizeof(double) * (21 * (size_t)c->K + 25), s));
    int rows = 0;
    { TimedScope t(c, I3D_K_EG_AUX); rows = launch_eg_gradcol(s, g, r, p, gb);
      if (rows > GC_PART_ROWS) return ctx_fail(c, I3D_ERR_CAPACITY, "run_gradcol: more workgroups than rows of the camera partial buffer");
      if (rows > 0) launch_sum_rows(s, PASS_COLNORM, c->K, c->gc_part.p + col_off, rows, stride, c->d_shared.p, c->d_blocks.p); }
    { PassBuffers b{c->C2.p, c->treg2.p, c->d_shared.p, c->d_blocks.p, nullptr, 0};
      TimedScope t(c, I3D_K_GATHER); launch_gather(s, PASS_COLNORM, r, b, c->v_c.p); }
    { TimedScope t(c, I3D_K_VECTOR); launch_shared_finalize(s, L.tail_off, c->K, p, c->d_shared.p, c->v_c.p, false, nullptr, nullptr, nullptr, nullptr, nullptr); }
    { int rc = between(); if (rc) return rc; }
    CTX_HIP(c, hipMemsetAsync(c->d_shared.p, 0, sizeof(double) * ((size_t)L.NS + 1), s));
    { TimedScope t(c, I3D_K_EG_AUX); if (rows > 0) launch_sum_rows(s, PASS_GRAD, c->K, c->gc_part.p, rows, stride, c->d_shared.p, c->d_blocks.p); }
    { PassBuffers b{c->C.p, c->treg.p, c->d_shared.p, c->d_blocks.p, nullptr, 0};
      TimedScope t(c, I3D_K_GATHER); launch_gather(s, PASS_GRAD, r, b, c->v_acc.p); }
    { TimedScope t(c, I3D_K_VECTOR); launch_shared_finalize(s, L.tail_off, c->K, p, c->d_shared.p, c->v_acc.p, false, nullptr, nullptr, nullptr, nullptr, nullptr); }
    return I3D_OK;
}

// a.b over the distributed vector: own slice -> all-reduce -> + the replicated camera tail; the result stays on the device (*slot, one of d_scal's doubles)
int dot_dev(i3d_context* c, const float* a, const float* b, double* slot) {
    const Layout L = layout_of(c);
    CTX_HIP(c, hipMemsetAsync(slot, 0, sizeof(double), c->stream));
    { TimedScope t(c, I3D_K_VECTOR); launch_dot2(c->stream, L.own, a, b, slot, c->d_partials.p); }
    { int rc = allreduce(c, slot, 1); if (rc) return rc; }
    { TimedScope t(c, I3D_K_VECTOR); launch_dot(c->stream, L.NS, a + L.tail_off, b + L.tail_off, slot, c->d_partials.p); }
    return I3D_OK;
}

// slot = number of owned entries (+ the replicated camera tail, counted once) with |a m| > tol
int count_above_dev(i3d_context* c, const float* a, const float* m, float tol, double* slot) {
    const Layout L = layout_of(c);
    CTX_HIP(c, hipMemsetAsync(slot, 0, sizeof(double), c->stream));
    { TimedScope t(c, I3D_K_VECTOR); launch_count_above2(c->stream, L.own, a, m, tol, slot, c->d_partials.p); }
    { int rc = allreduce(c, slot, 1); if (rc) return rc; }
    { TimedScope t(c, I3D_K_VECTOR); launch_count_above(c->stream, L.NS, a + L.tail_off, m + L.tail_off, tol, slot, c->d_partials.p); }
    return I3D_OK;
}

int eval_cost_launch(i3d_context* c, const OptParams& p, bool candidate, const FrameConst* frames, const double* cam9, const LmState* lm) {
    GridView g = c->grid_view();
    if (candidate) { g.x_sdf = c->xc_sdf.p; g.x_alb = c->xc_alb.p; }
    { TimedScope t(c, I3D_K_COST); launch_build(c->stream, g, c->row_view(), p, frames, false, c->d_scal.p + 16, c->d_partials.p, cam9, lm); }
    return allreduce(c, c->d_scal.p + 16, 1);
}

// ---- the pass protocol of the three drivers ----------------------------------------------------------------------------------------------------------
constexpr int PCG_MAX_ITERATIONS = 500;     // the stopping rule's iteration limit (k_pcg_init*)
constexpr int PCG_MAX_PASSES = 520;         // what a host queues at most: the limit + the passes queued behind a convergence flag it has not seen yet
constexpr int PCG_RESET_PERIOD = 10;        // residual_reset_period: every tenth pass forms r = b - A x instead of r -= alpha q
constexpr int PCG_SEQ_STRIDE = 1024;        // pass numbers a PCG solve may use (<= 521 passes): the numbering of the next solve does not depend on how many passes a host queued

// fp64 partial sums of a solve: the slice sums of the step kernel, then the p.q partials of the operator pass, then the D^2 p^2 partials of the direction kernel
// (at d_partials; a system of a ladder batch: at its slab of ladder.part)
constexpr int PART_STEP = 4 * 2048, PART_PQ = 2048, PART_D2 = 2048;
struct Partials { double *step, *pq, *d2; };
static Partials partials_at(double* base) { return Partials{base, base + PART_STEP, base + PART_STEP + PART_PQ}; }

// Wait until the boundary kernel of pass `want` has published itself in `ring` = (pass, done) of the mapped host flags: polled; after 30 s one synchronisation and a
// last look, then `stalled` is the error.  *done = the ring's done flag.
static int wait_pass(i3d_context* c, const int* ring, int want, const char* stalled, bool* done) {
    const double t_wait = now_s();
    while (__atomic_load_n(&ring[0], __ATOMIC_ACQUIRE) != want) {
        if (now_s() - t_wait > 30.0) { CTX_HIP(c, sync_stream(c)); if (__atomic_load_n(&ring[0], __ATOMIC_ACQUIRE) != want) return ctx_fail(c, I3D_ERR_HIP, stalled); }
    }
    *done = __atomic_load_n(&ring[1], __ATOMIC_ACQUIRE) != 0;
    return I3D_OK;
}
// the two single-system loops look at the boundary of pass it-1 while pass `it` (number `seq`) runs
static int previous_pass_done(i3d_context* c, int it, int seq, bool* done) {
    if (it < 2) return I3D_OK;
    return wait_pass(c, c->h_flags + 2 * ((seq - 1) & 1), seq - 1, "pcg_solve: the device stopped publishing its state", done);
}

// Pass numbers.  They are unique across solves, so a stale ring entry can never match, and they are the epochs of the in-kernel exchanges: identical on all ranks
// (every rank queues the same solves; how many passes a rank's HOST queued behind the convergence flag may differ, so every solve takes a fixed block of numbers).
// Pass `it` = 1, 2, ... of a solve has the number begin_passes() + it.
static int begin_passes(const i3d_context* c) { return c->pcg_seq; }
static void end_passes(i3d_context* c, int seq0) { c->pcg_seq = seq0 + PCG_SEQ_STRIDE; }

// u = S x on the owned segments and the camera tail: the operator input of a residual-reset pass (inside the caller's timed scope)
static void launch_u_from_x(i3d_context* c, const Layout& L, const float* x, float* u) {
    launch_mul2(c->stream, L.own, c->v_S.p, x, u); launch_mul(c->stream, L.NS, c->v_S.p + L.tail_off, x + L.tail_off, u + L.tail_off);
}

// CGNR (ConjugateGradientsSolver) on (S J^T W J S + D^2) x = b, x0 = 0.  No host synchronisation inside an iteration.  Six launches per pass.
// One rank: the untiled operator (k_eg_jtjp + k_gather).  Sharded (one process per GPU): the tiled operator; a rank iterates on its two owned segments of
// every vector + the replicated camera tail.  Per pass:
//   * ONE neighbour exchange: the operator input u = S p on the rim the rank's rows read (Comm::push_halo, a few tens of KB per pair);
//   * ONE small all-reduce after the operator: [camera block 6K+9 | p.q] (fp64);
//   * ONE all-reduce of the 4 iteration scalars (r.z, x.(b+r), x.r, sum D^2 x^2) at the iteration boundary.
// No vector is gathered: everything that lands on an owned unknown is computed from rows the rank holds itself (owned + ghost entries).
// The terminal state stays on the device: k_lm_decide reads it on the stream.
int pcg_solve(i3d_context* c, const SolveRoute& route, const i3d_optimizer_config& cfg, const OptParams& p, const PcgState** final_state) {
    hipStream_t s = c->stream;
    const Layout L = layout_of(c);
    const int K = c->K;
    const bool sh = c->sharded();      // = the tiled operator: on one rank this loop runs the untiled pass only (solve_route)
    GridView g = c->grid_view(); RowView r = c->row_view();
    PassBuffers pb{c->C.p, c->treg.p, c->d_shared.p, c->d_blocks.p, c->aux_part.p, (int)aux_part_stride(c->K)};
    PcgState* st = c->d_pcg.p;
    double* pq_slot = c->d_shared.p + L.NS;
    const size_t to = L.tail_off; const Seg2 own = L.own;
    { TimedScope t(c, I3D_K_VECTOR); launch_fill(s, (int)L.NP, c->v_x.p, 0.0f); launch_pcg_init(s, st, cfg.pcg_fixed_iterations, PCG_MAX_ITERATIONS, c->d_lm.p); }
    CTX_HIP(c, hipMemcpyAsync(c->v_r.p, c->v_b.p, sizeof(float) * L.NP, hipMemcpyDeviceToDevice, s));
    const Partials part = partials_at(c->d_partials.p);
    int n_pq = 0, n_step = 0, n_d2 = 0;
    // Sharded over the peer-to-peer transport: the two reductions of a pass run INSIDE the boundary kernels (k_pcg_tail_a / k_pcg_tail_b), a pass
    // has no reduction launches of its own.  Any other transport: separate all-reduce launches around the same kernels (pd.on = 0).
    const bool dev_reduce = route.exchange == Exchange::InKernelReduce;
    const P2PDev& pd = route.reduce_dev;
    // The operator on the rows of this rank.  Tiled (tile_pass.hip): raw accumulators J^T W J u in v_qacc (camera block in d_shared, p.q partials
    // row by row); the vector q = S acc + D^2 v is formed inside k_pcg_step.  Untiled fallback (single rank): k_eg_jtjp + k_gather -> out.
    auto rows_apply = [&](const float* v, float* out, bool with_dot, bool zero_first) -> int {
        if (zero_first) CTX_HIP(c, hipMemsetAsync(c->d_shared.p, 0, sizeof(double) * ((size_t)L.NS + 1), s));      // (the pass boundary kernel zeroes it otherwise)
        if (sh) {
            { int rc = push_halo(c, c->v_u.p); if (rc) return rc; }
            { TimedScope t(c, I3D_K_EG_PASS);
              n_pq = launch_eg_tile(s, r, p, c->v_u.p, c->tile_plan(), c->d_shared.p, c->v_qacc.p, with_dot ? part.pq : nullptr, st); }
            { TimedScope t(c, I3D_K_GATHER); launch_halo_fold(s, r, c->tile_plan(), c->v_qacc.p, st); }
            if (!with_dot) n_pq = 0;
            if (dev_reduce && with_dot) return I3D_OK;      // k_pcg_tail_b adds the partials and sums [camera block | p.q] over the ranks
            // the rank's p.q (rows + D^2 p^2 of its slice) rides with the camera block
            if (with_dot) { TimedScope t(c, I3D_K_VECTOR); launch_reduce_partials(s, part.pq, n_pq, 1, pq_slot, st); launch_reduce_partials(s, part.d2, n_d2, 1, pq_slot, st); }
            n_pq = 0;
            return allreduce(c, c->d_shared.p, (size_t)L.NS + 1);
        }
        { TimedScope t(c, I3D_K_EG_PASS); launch_eg_pass(s, PASS_JTJP, g, r, p, c->v_u.p, pb, st); }
        { TimedScope t(c, I3D_K_GATHER); n_pq = launch_gather_tail(s, r, pb, out, c->v_S.p, c->v_D2.p, v, with_dot ? part.pq : nullptr, false, st); }
        if (!with_dot) n_pq = 0;
        return I3D_OK;
    };
    // sharded: the slice sums of k_pcg_step go into acc (one small launch: thousands of workgroups adding into four doubles serialise at the L2,
    // measured 71 vs 32 us for the step kernel), which is all-reduced at the iteration boundary; single rank: k_pcg_tail_a adds the partials itself
    auto fold_step = [&]() { if (sh && !dev_reduce) { launch_reduce_partials(s, part.step, n_step, 4, st->acc, st); n_step = 0; } };
    const float* const Sq = sh ? c->v_S.p : nullptr;          // tiled pass: k_pcg_step forms q from the accumulators
    { TimedScope t(c, I3D_K_VECTOR);
      n_step = launch_pcg_step(s, 0 /*init*/, own, c->v_p.p, c->v_q.p, c->v_x.p, c->v_r.p, c->v_b.p, c->v_D2.p, c->v_Minv.p, c->v_z.p, nullptr, part.step, st);
      fold_step(); }
    int tail_mode = 0;
    const int seq0 = begin_passes(c);
    for (int it = 1;; ++it) {
        // iteration boundary.  Sharded: the 4 slice sums (r.z, x.(b+r), x.r, sum D2 x^2) are summed over the ranks — inside k_pcg_tail_a over the
        // mailbox transport, by a reduction + all-reduce launch otherwise
        if (sh && !dev_reduce) { int rc = allreduce(c, st->acc, 4); if (rc) return rc; }
        if (dev_reduce) { c->comm->count_reduce(4); c->comm->count_reduce((size_t)L.NS + 1); }
        { TimedScope t(c, I3D_K_VECTOR);
          launch_pcg_tail_a(s, tail_mode, to, K, c->Minv_blocks.p, c->v_p.p, tail_mode == 3 ? c->v_tmp.p : c->v_q.p, c->v_x.p, c->v_r.p, c->v_b.p, c->v_D2.p, c->v_z.p,
                            part.step, n_step, st, c->d_shared.p, L.NS + 1, c->d_flags, seq0 + it, pd); }
        { TimedScope t(c, I3D_K_VECTOR);        // p = z + beta p, u = S p on the owned segments and the (replicated) camera tail; sharded: D^2 p^2 of the tail is added by k_pcg_tail_b
          n_d2 = launch_pcg_direction(s, own, to, L.NS, c->v_z.p, c->v_p.p, c->v_S.p, c->v_u.p, c->v_D2.p, sh ? part.d2 : nullptr, st); }
        { int rc = rows_apply(c->v_p.p, c->v_q.p, true, false); if (rc) return rc; }
        { TimedScope t(c, I3D_K_VECTOR); launch_pcg_tail_b(s, to, K, p, c->d_shared.p, pq_slot, part.pq, n_pq, part.d2, dev_reduce ? n_d2 : 0, sh,
                                                           c->v_q.p, c->v_S.p, c->v_D2.p, c->v_p.p, st, pd); }
        if (it % PCG_RESET_PERIOD != 0) {
            TimedScope t(c, I3D_K_VECTOR);
            n_step = launch_pcg_step(s, 1, own, c->v_p.p, sh ? c->v_qacc.p : c->v_q.p, c->v_x.p, c->v_r.p, c->v_b.p, c->v_D2.p, c->v_Minv.p, c->v_z.p, Sq, part.step, st);
            fold_step();
            tail_mode = 1;
        } else {                                                                 // r = b - A x instead of r -= alpha q
            { TimedScope t(c, I3D_K_VECTOR);
              launch_pcg_step(s, 2, own, c->v_p.p, c->v_q.p, c->v_x.p, c->v_r.p, c->v_b.p, c->v_D2.p, c->v_Minv.p, c->v_z.p, nullptr, part.step, st);
              launch_pcg_tail_x(s, to, K, c->v_p.p, c->v_x.p, st);
              launch_u_from_x(c, L, c->v_x.p, c->v_u.p); }
            { int rc = rows_apply(c->v_x.p, c->v_tmp.p, false, true); if (rc) return rc; }
            { TimedScope t(c, I3D_K_VECTOR);
              launch_shared_finalize(s, to, K, p, c->d_shared.p, c->v_tmp.p, true, c->v_S.p, c->v_D2.p, c->v_x.p, nullptr, st);
              n_step = launch_pcg_step(s, 3, own, c->v_p.p, sh ? c->v_qacc.p : c->v_tmp.p, c->v_x.p, c->v_r.p, c->v_b.p, c->v_D2.p, c->v_Minv.p, c->v_z.p, Sq, part.step, st);
              fold_step(); }
            tail_mode = 3;
        }
        bool done = false;
        { const int rc = previous_pass_done(c, it, seq0 + it, &done); if (rc) return rc; }
        if (done || it > PCG_MAX_PASSES) break;
    }
    end_passes(c, seq0);
    *final_state = st;                   // kernels after `done` were no-ops, so this is the terminal state (read by k_lm_decide on the stream)
    return I3D_OK;
}

// The arguments of k_pcg_step3 that pcg_solve_fused and pcg_solve_ladder fill alike.  x / r / pv / z / q: the vectors of the solve (a ladder batch: those of its system 0,
// the others follow at the slab strides); qh: the halo sums the operator leaves; part: the partial sums; cam, Mblk, tD2: camera partial rows, block-Jacobi
// inverses and LM diagonal of the camera tail.  The caller adds what only it has: sharded + sh, lad_sys, redop.
static Step3Args step3_args(const i3d_context* c, const Layout& L, const OptParams& p, const TilePlan& tp, float* x, float* r, float* pv, float* z, const float* q, const float* qh,
                            const Partials& part, const float* cam, const float* Mblk, const float* tD2, int wg_cap) {
    const Seg2 own = L.own; const size_t to = L.tail_off;
    Step3Args a; std::memset(&a, 0, sizeof(a));
    auto c4 = [&](const float* v) { return reinterpret_cast<const float4*>(v + own.off0); };
    auto m4 = [&](float* v) { return reinterpret_cast<float4*>(v + own.off0); };
    a.nq = own.n >> 2; a.chunk4 = (int)((own.off1 - own.off0) >> 2);
    a.p = c4(pv); a.qacc = c4(q); a.x = m4(x); a.r = m4(r); a.b = c4(c->v_b.p); a.z = m4(z); a.cm = c4(c->v_cm.p); a.lm = c->d_lm.p;
    a.ext_off = tp.ext_off; a.ext_pos = tp.ext_pos; a.qh = reinterpret_cast<const float2*>(qh); a.e0 = (int)own.off0;
    a.pq_partials = part.pq; a.d2_partials = part.d2; a.n_pq = 0; a.n_d2 = 0;
    a.n_slice_wg = pcg_step3_slice_wgs(own.n, wg_cap);
    a.K = c->K; a.fix_poses = p.fix_poses; a.fix_intr = p.fix_intr; a.fix_dist = p.fix_dist;
    a.cam_partials = cam; a.n_cam = 0; a.cam_stride = (L.NS + 3) & ~3; a.Mblk = Mblk;
    a.tp = pv + to; a.tx = x + to; a.tr = r + to; a.tb = c->v_b.p + to; a.tD2 = tD2; a.tz = z + to; a.tS = c->v_S.p + to;
    a.step_partials = part.step;
    return a;
}

// The same solve in THREE launches per pass (pcg_fused.hip): k_pcg_dir3 | k_eg_tile | k_pcg_step3.  Single rank, tiled operator.  The scalar state is
// double-buffered by pass parity: boundary `it` reads st2[(it + 1) & 1] and writes st2[it & 1], which the operator and the step of pass `it` read.
// Sharded (one process per GPU, mailbox transport): the SAME three launches — the boundary's exchange ([4 slice sums] + the rim of z) runs inside k_pcg_dir3, the
// operator's ([p.q | camera block]) inside k_pcg_step3; the residual-reset passes (one in ten) push the rim of u = S x with a launch of their own (k_rim_u).
int pcg_solve_fused(i3d_context* c, const SolveRoute& route, const i3d_optimizer_config& cfg, const OptParams& p, const PcgState** final_state) {
    hipStream_t s = c->stream;
    const Layout L = layout_of(c);
    const size_t to = L.tail_off; const Seg2 own = L.own;
    RowView r = c->row_view(); TilePlan tp = c->tile_plan();
    const bool sh = route.exchange == Exchange::InKernel;
    ShardArgs sa; std::memset(&sa, 0, sizeof(sa));
    if (sh) {
        if (!c->comm->fused_exchange(&sa.pd) || L.NS + 2 > sa.pd.L.red_cap) return ctx_fail(c, I3D_ERR_STATE, "pcg_solve_fused: the in-kernel exchanges are not available");
        const ShardState& sd = c->shard; const HaloPlan& h = sd.halo;
        sa.rim = RimLists{h.n_send, h.n_recv, sd.halo_send_idx.p, sd.halo_send_peer.p, sd.halo_recv_idx.p, sd.halo_recv_peer.p, sd.halo_offs.p, sd.halo_offs.p + P2P_MAX_RANKS};
        sa.n_rim_wg = (h.n_send + h.n_recv) > 0 ? std::max(1, std::min(4, (std::max(h.n_send, h.n_recv) + 1023) / 1024)) : 1;
        sa.zb = c->v_z.p; sa.pb = c->v_p.p; sa.ub = c->v_u.p; sa.cmb = c->v_cm.p; sa.chunk = sd.chunk;
    }
    const int wg_cap = sh ? sa.pd.wg_cap : 0;
    PcgState* const st2 = c->d_pcg2.p;
    const int NSP = (L.NS + 3) & ~3;
    const Partials part = partials_at(c->d_partials.p);
    { TimedScope t(c, I3D_K_VECTOR); launch_fill(s, (int)L.NP, c->v_x.p, 0.0f); launch_pcg_init3(s, st2, cfg.pcg_fixed_iterations, PCG_MAX_ITERATIONS, c->d_lm.p); }
    CTX_HIP(c, hipMemcpyAsync(c->v_r.p, c->v_b.p, sizeof(float) * L.NP, hipMemcpyDeviceToDevice, s));
    Step3Args a = step3_args(c, L, p, tp, c->v_x.p, c->v_r.p, c->v_p.p, c->v_z.p, c->v_qacc.p, tp.qh, part, c->cam_part.p, c->Minv_blocks.p, c->v_D2.p + to, wg_cap);
    a.sharded = sh ? 1 : 0; a.lad_sys = -1;
    int n_step = 0;
    { TimedScope t(c, I3D_K_VECTOR); a.cur = st2; n_step = launch_pcg_step3(s, 0 /*init*/, a); }
    const bool mr1 = c->op.mr1_serial && !sh && route.multi_system;
    auto op = [&](double* pq, const PcgState* cur) -> int {      // q_acc = J^T W J u on the rows of this rank
        if (mr1) { const int sys0[3] = {0, 0, 0}; LadVec z; std::memset(&z, 0, sizeof(z));
                   return launch_eg_tile_mr(s, r, p, tp, 1, sys0, c->v_u.p, c->v_qacc.p, tp.qh, pq, c->cam_part.p, NSP, cur, z); }
        return launch_eg_tile(s, r, p, c->v_u.p, tp, nullptr, c->v_qacc.p, pq, cur, c->cam_part.p, NSP);
    };
    const int seq0 = begin_passes(c);
    int it = 1;
    for (;; ++it) {
        PcgState* const prev = st2 + ((it + 1) & 1); PcgState* const cur = st2 + (it & 1);
        sa.seq = seq0 + it; sa.n_slice_partials = a.n_slice_wg; a.sh = sa;
        { TimedScope t(c, I3D_K_VECTOR);
          a.n_d2 = launch_pcg_dir3(s, it == 1, own, to, L.NS, c->v_z.p, c->v_p.p, c->v_S.p, c->v_u.p, c->v_D2.p, c->v_cm.p, c->d_lm.p, part.step, n_step, part.d2, prev, cur, c->d_flags, seq0 + it,
                                   sh ? &sa : nullptr); }
        if (sh) { c->comm->count_reduce(4); c->comm->count_halo(c->shard.halo.n_send); c->comm->count_reduce((size_t)L.NS + 1); }      // (logged as exchanges of this pass: they have no launches of their own)
        { TimedScope t(c, I3D_K_EG_PASS); a.n_pq = op(part.pq, cur); a.n_cam = a.n_pq; }
        a.cur = cur;
        if (it % PCG_RESET_PERIOD != 0) { TimedScope t(c, I3D_K_VECTOR); n_step = launch_pcg_step3(s, 1, a); }
        else {                                                                   // r = b - A x instead of r -= alpha q
            { TimedScope t(c, I3D_K_VECTOR); launch_pcg_step3(s, 2, a); launch_u_from_x(c, L, c->v_x.p, c->v_u.p); }
            if (sh) { TimedScope t(c, I3D_K_COMM); launch_rim_u(s, sa, cur); c->comm->count_halo(c->shard.halo.n_send); }
            { TimedScope t(c, I3D_K_EG_PASS); a.n_cam = op(nullptr, cur); }
            { TimedScope t(c, I3D_K_VECTOR); n_step = launch_pcg_step3(s, 3, a); }
        }
        bool done = false;
        { const int rc = previous_pass_done(c, it, seq0 + it, &done); if (rc) return rc; }
        if (done || it > PCG_MAX_PASSES) break;
    }
    end_passes(c, seq0);
    // boundary `it` copied the terminal state forward (kernels after `done` are no-ops), so st2[it & 1] is final (read by k_lm_decide on the stream)
    *final_state = st2 + (it & 1);
    { const int lrc = ctx_launch_check(c); if (lrc) return lrc; }
    return I3D_OK;
}

// ---- the damping ladder ------------------------------------------------------------------------------------------------------------------------------
// Slabs of the per-system arrays of a batch (LadVec): every system has its own x, r, p, z, u, operator accumulators, halo sums, camera partial rows, partial
// sums, block-Jacobi inverses, camera-tail diagonal and scalar states; b, the column norms and S are shared.
static size_t lad_redop_stride(int NS) { return ((size_t)NS + 1 + 3) & ~(size_t)3; }
// Sized by what the CURRENT work list needs (round 6, advisor finding of round 5: the slabs were sized by the whole grid — 2.3 GB of vectors + 1.2 GB of halo sums at the bench
// size, 290 bytes per stored voxel on top of the 16 solver vectors, whatever the active share): the vectors by the list's layout (2 chunk + 6K + 9, rounded up to 64 K entries so
// that a list that grows a little does not reallocate), the halo sums by the list's tiles.  Grow-only.  Returns non-zero WITHOUT latching an error when the device cannot hold
// them: the caller then solves this outer iteration with the serial trust-region loop.
int alloc_ladder(i3d_context* c) {
    const Layout L = layout_of(c);
    const int nsys = c->op.ladder_max;
    LadderState& ld = c->ladder; LadVec& lv = ld.strides;
    const size_t vec = ((size_t)L.NP + 65535) & ~(size_t)65535;
    const size_t qh = 2 * (size_t)tile_plan_tiles_of((int)std::min((size_t)c->Acap, ((size_t)c->shard.chunk + 65535) & ~(size_t)65535), 512) * (size_t)tile_plan_hmax_of(512);
    const size_t cam = (size_t)2048 * (((size_t)L.NS + 3) & ~(size_t)3);
    lv.vec = vec; lv.qh = qh; lv.cam = cam; lv.part = PART_STEP + PART_PQ + PART_D2; lv.mblk = ((size_t)36 * c->K + 41 + 3) & ~(size_t)3; lv.tail = ((size_t)L.NS + 3) & ~(size_t)3;
    const bool fresh = ld.vec.n < (size_t)6 * nsys * vec || !ld.vec.p;
    bool ok = ld.vec.alloc((size_t)6 * nsys * vec) == hipSuccess;
    if (ok && fresh) ok = hipMemsetAsync(ld.vec.p, 0, sizeof(float) * ld.vec.n, c->stream) == hipSuccess;      // padding entries stay finite
    ok = ok && ld.qh.alloc((size_t)nsys * qh) == hipSuccess && ld.cam.alloc((size_t)nsys * cam) == hipSuccess && ld.part.alloc((size_t)nsys * lv.part) == hipSuccess
            && ld.mblk.alloc((size_t)nsys * lv.mblk) == hipSuccess && ld.tail.alloc((size_t)nsys * lv.tail) == hipSuccess && ld.st.alloc((size_t)2 * LADDER_MAX) == hipSuccess;
    if (ok && c->sharded()) {      // what a pass all-reduces: [LADDER_MAX][4] slice sums of the step kernel, then [LADDER_MAX][NS + 1, padded] camera block + p.q of the operator pass
        const size_t n = (size_t)LADDER_MAX * (4 + lad_redop_stride(L.NS));
        const bool fresh_r = ld.red.n < n || !ld.red.p;
        ok = ld.red.alloc(n) == hipSuccess;
        if (ok && fresh_r) ok = hipMemsetAsync(ld.red.p, 0, sizeof(double) * ld.red.n, c->stream) == hipSuccess;      // slots of systems that are not live are summed too: keep them finite
    }
    if (!ok) {
        (void)hipGetLastError();
        ld.vec.release(); ld.qh.release(); ld.cam.release(); ld.part.release();
        std::fprintf(stderr, "[i3d] the slabs of the damping ladder (%d systems x %.1f MB) do not fit the device: this outer iteration runs the serial trust-region loop\n", nsys,
                     (double)(6 * vec + qh + cam) * 4.0 / 1e6);
        return 1;
    }
    return I3D_OK;
}

// B systems (J^T W J + D_j^2) y = b, j = 0 .. B-1 (the LM diagonals of a ladder batch, k_lm_begin_lad), iterated in LOCK STEP: pass `it` of the loop is iteration `it` of
// every system still running.  Per pass: ONE k_pcg_dir3 launch and ONE k_pcg_step3 launch over the live systems (blockIdx.y), and the operator — the rows are streamed
// once per GROUP of up to 3 live systems (k_eg_tile_mr) instead of once per system.  Every system keeps its own scalar state, stopping rule and host ring; a system
// that has stopped is dropped from the launches one pass after the host saw its flag.  The arithmetic of a system is that of pcg_solve_fused on it alone.
int pcg_solve_ladder(i3d_context* c, const SolveRoute& route, const i3d_optimizer_config& cfg, const OptParams& p, int B, const PcgState** finals) {
    hipStream_t s = c->stream;
    const Layout L = layout_of(c);
    const int K = c->K; const size_t to = L.tail_off; const Seg2 own = L.own;
    RowView r = c->row_view(); TilePlan tp = c->tile_plan();
    LadderState& ld = c->ladder; LadVec lv = ld.strides;
    float* const X0 = lad_vecp(c, LV_X); float* const R0 = lad_vecp(c, LV_R); float* const P0 = lad_vecp(c, LV_P); float* const Z0 = lad_vecp(c, LV_Z);
    float* const U0 = lad_vecp(c, LV_U); float* const Q0 = lad_vecp(c, LV_Q);
    PcgState* const st2 = ld.st.p;
    const int NSP = (L.NS + 3) & ~3;
    const Partials part0 = partials_at(ld.part.p);      // of system 0; the others follow at lv.part
    const bool use_mr = c->sw.ladder_mr;        // I3D_LADDER_MR=0: the single-system operator once per system (A/B and parity runs)
    const bool mr1 = c->sw.ladder_mr1;          // I3D_LADDER_MR1=1: a lone live system goes through k_eg_tile_mr<1> as well
    const int mr_cap = std::min(c->sw.ladder_group, eg_tile_mr_max_systems(K));
    const bool pair = c->sw.ladder_pair;        // I3D_LADDER_PAIR=0: a pass of two groups is two launches, each a stream of the rows from HBM (A/B and parity runs)
    const bool mr_ok = use_mr && mr_cap >= 1 && route.multi_system;
    // Sharded (exchanges as launches of the transport: RCCL, the rank simulation).  Per pass and BATCH, not per system:
    //   k_lad_reduce_step + ONE all-reduce of [LADDER_MAX][4] doubles (the slice sums of every live system) in front of k_pcg_dir3_lad,
    //   the rim of u = S p of every live system pushed after it (one exchange per system: the transport's lists are per vector),
    //   k_lad_reduce_op + ONE all-reduce of [LADDER_MAX][6K + 10] doubles (camera block + p.q of every live system) behind the operator.
    // The slots of systems that have stopped ride along unused: the message size does not depend on which systems are live, so the ranks' collectives always match.
    const bool sh = route.exchange == Exchange::Transport;
    // (without the multi-system pass — I3D_LADDER_MR=0 — a sharded batch streams its rows once per system through k_eg_tile<..., GHOSTS>, like a single-rank one: the exchanges stay batched)
    double* const red4 = sh ? ld.red.p : nullptr;
    const int rstride = (int)lad_redop_stride(L.NS);
    double* const redop = sh ? ld.red.p + (size_t)LADDER_MAX * 4 : nullptr;
    { TimedScope t(c, I3D_K_VECTOR);
      for (int j = 0; j < B; ++j) { CTX_HIP(c, hipMemsetAsync(X0 + (size_t)j * lv.vec, 0, sizeof(float) * L.NP, s));
                                    CTX_HIP(c, hipMemcpyAsync(R0 + (size_t)j * lv.vec, c->v_b.p, sizeof(float) * L.NP, hipMemcpyDeviceToDevice, s)); }
      launch_pcg_init_lad(s, st2, B, cfg.pcg_fixed_iterations, PCG_MAX_ITERATIONS, c->d_lm.p); }
    Step3Args a = step3_args(c, L, p, tp, X0, R0, P0, Z0, Q0, ld.qh.p, part0, ld.cam.p, ld.mblk.p, ld.tail.p, 0);
    a.sharded = 0; a.lad_sys = 0; a.redop = redop; a.redop_stride = rstride;
    std::vector<int> live(B); for (int j = 0; j < B; ++j) live[j] = j;
    auto set_slots = [&]() { for (int q = 0; q < LADDER_MAX; ++q) lv.sysid[q] = live[q < (int)live.size() ? q : (int)live.size() - 1]; };
    // the operator on the live systems: groups of <= mr_cap systems share one stream of the rows; returns the workgroups per system (p.q partials / camera rows)
    auto rows_apply = [&](int parity, bool with_dot) -> int {
        int n = 0; const int nl = (int)live.size();
        if (sh) { TimedScope t(c, I3D_K_COMM);      // the rim of every live system's operator input: ONE message per peer, nl values per entry
                  if (c->comm->push_halo_multi(U0, lv.vec, live.data(), nl, c->shard.halo, s)) return -1; }
        if (mr_ok && (nl > 1 || mr1 || sh)) {
            const int groups = (nl + mr_cap - 1) / mr_cap;
            int at = 0;
            // Two groups (4 .. 6 live systems at three per group): ONE launch whose paired workgroups share an XCD — the second group's rows come out of the cache the
            // first group's read filled (tile_pass_mr.hip, PAIR).  Timed under the category of the wider group: the launch is one stream of the rows, as the byte model of
            // the benchmark prices it, but it does the arithmetic of both groups, so the category's time per launch rises.  Single rank; 0 = not available.
            if (groups == 2 && pair && !sh && nl - (nl + 1) / 2 >= 2) {
                const int na = (nl + 1) / 2;
                TimedScope t(c, na == 2 ? I3D_K_EG_MR2 : I3D_K_EG_MR3);
                n = launch_eg_tile_mr_pair(s, r, p, tp, na, nl - na, live.data(), U0, Q0, ld.qh.p, with_dot ? part0.pq : nullptr, ld.cam.p, NSP, st2 + parity, lv);
                if (n > 0) { at = nl; ++ld.streams; ++ld.paired; }
            }
            for (int g = 0; g < groups && at < nl; ++g) {
                const int ng = (nl - at + (groups - g) - 1) / (groups - g);        // balanced: 4 -> 2 + 2, 5 -> 3 + 2
                TimedScope t(c, ng == 1 ? I3D_K_EG_PASS : (ng == 2 ? I3D_K_EG_MR2 : I3D_K_EG_MR3));
                n = launch_eg_tile_mr(s, r, p, tp, ng, live.data() + at, U0, Q0, ld.qh.p, with_dot ? part0.pq : nullptr, ld.cam.p, NSP, st2 + parity, lv);
                if (n <= 0) return -1;
                at += ng; ++ld.streams;
            }
        } else {
            for (int j : live) {
                TilePlan tj = tp; tj.qh = ld.qh.p + (size_t)j * lv.qh;
                TimedScope t(c, I3D_K_EG_PASS);
                n = launch_eg_tile(s, r, p, U0 + (size_t)j * lv.vec, tj, nullptr, Q0 + (size_t)j * lv.vec, with_dot ? part0.pq + (size_t)j * lv.part : nullptr, st2 + 2 * j + parity,
                                   ld.cam.p + (size_t)j * lv.cam, NSP);
                ++ld.streams;
            }
        }
        ld.system_passes += nl; ++ld.pass_live[nl < 6 ? nl : 6];
        if (sh) {          // this rank's [camera block | p.q (+ D^2 p^2 of its slice)] of every live system -> summed over the ranks, one message
            { TimedScope t(c, I3D_K_VECTOR); launch_lad_reduce_op(s, nl, ld.cam.p, n, NSP, L.NS, part0.pq, with_dot ? n : 0, part0.d2, with_dot ? a.n_d2 : 0, redop, rstride, lv); }
            if (allreduce(c, redop, (size_t)LADDER_MAX * rstride)) return -1;
        }
        return n;
    };
    // sharded: the four slice sums of every live system, summed over the ranks in front of the boundary kernel
    auto step_sums = [&](int nl, int n_slice) -> int {
        if (!sh) return I3D_OK;
        { TimedScope t(c, I3D_K_VECTOR); launch_lad_reduce_step(s, nl, part0.step, n_slice, red4, lv); }
        return allreduce(c, red4, (size_t)LADDER_MAX * 4);
    };
    int n_step = 0;
    set_slots();
    { TimedScope t(c, I3D_K_VECTOR); a.cur = st2; n_step = launch_pcg_step3_lad(s, 0 /*init*/, B, a, lv); }
    for (int j = 0; j < B; ++j) finals[j] = st2 + 2 * j;
    const int seq0 = begin_passes(c);
    int it = 1;
    for (;; ++it) {
        set_slots();
        const int nl = (int)live.size();
        { const int rc = step_sums(nl, a.n_slice_wg); if (rc) return rc; }
        { TimedScope t(c, I3D_K_VECTOR);
          a.n_d2 = launch_pcg_dir3_lad(s, it == 1, nl, own, to, L.NS, Z0, P0, c->v_S.p, U0, ld.tail.p, c->v_cm.p, c->d_lm.p, part0.step, n_step, part0.d2, st2, (it + 1) & 1, c->d_flags, seq0 + it, lv,
                                       a.n_slice_wg, red4); }
        { const int n = rows_apply(it & 1, true); if (n < 0) return ctx_fail(c, I3D_ERR_STATE, "pcg_solve_ladder: the multi-system operator pass could not be launched"); a.n_pq = n; a.n_cam = n; }
        a.cur = st2 + (it & 1);
        if (it % PCG_RESET_PERIOD != 0) { TimedScope t(c, I3D_K_VECTOR); n_step = launch_pcg_step3_lad(s, 1, nl, a, lv); }
        else {                                                                   // r = b - A x instead of r -= alpha q
            { TimedScope t(c, I3D_K_VECTOR); launch_pcg_step3_lad(s, 2, nl, a, lv);
              for (int j : live) launch_u_from_x(c, L, X0 + (size_t)j * lv.vec, U0 + (size_t)j * lv.vec); }
            { const int n = rows_apply(it & 1, false); if (n < 0) return ctx_fail(c, I3D_ERR_STATE, "pcg_solve_ladder: the multi-system operator pass could not be launched"); a.n_cam = n; }
            { TimedScope t(c, I3D_K_VECTOR); n_step = launch_pcg_step3_lad(s, 3, nl, a, lv); }
        }
        {   // The boundary of THIS pass (k_pcg_dir3_lad of pass `it`, queued above), system by system.  Round 5 looked one pass further back (the boundary of pass it-1, after
            // queueing pass it): a system that had stopped was carried through TWO more passes — its slot in a stream of the rows (a dead system still stages its inputs, and
            // keeps the launch at its wider variant) — 103.6 system passes per iteration on the driver's protocol against the 83.5 the PCG iteration counts add up to.  Waiting
            // for this pass's own boundary costs nothing on the device: it is queued behind pass it-1, whose operator and step kernels are still running or queued when the host
            // gets here, and pass it+1 is queued while the operator of pass `it` runs.  A stopped system is carried through ONE pass (the rest of this one).
            const int want = seq0 + it;
            std::vector<int> still;
            for (int j : live) {
                bool done = false;
                { const int rc = wait_pass(c, c->h_flags + 4 * j + 2 * (want & 1), want, "pcg_solve_ladder: the device stopped publishing its state", &done); if (rc) return rc; }
                if (!done) still.push_back(j);
                else finals[j] = st2 + 2 * j + (it & 1);       // boundary `it` wrote the terminal state into this pass's buffer; no later boundary copies it into the other
            }
            live.swap(still);
        }
        if (live.empty() || it > PCG_MAX_PASSES) break;
    }
    end_passes(c, seq0);
    for (int j : live) finals[j] = st2 + 2 * j + (it & 1);       // (only after the pass limit: the state of the last pass queued)
    { const int lrc = ctx_launch_check(c); if (lrc) return lrc; }
    return I3D_OK;
}

}  // namespace i3d
