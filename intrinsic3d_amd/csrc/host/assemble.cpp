// The assembly of one outer iteration on the device:
//   assemble()  = Optimizer::addVoxelResiduals over all voxels + NLSSolver::buildProblem (optimizer.cpp:119-165, nls_solver.cpp:190-276)
// the work list, the operator plan (which pass, which tile geometry), the sharding plan of a multi-rank run, the rows and their weight sums.
#include "solver_internal.hpp"
#include <rocprim/rocprim.hpp>
#include <algorithm>

namespace i3d {

static OptParams make_params(const i3d_context* c, const i3d_optimizer_config& cfg) {
    OptParams p = camera_params(c, cfg.rgbd_level, cfg.occlusion_distance);
    p.thres_shell = cfg.thres_shell; p.lambda_a = cfg.lambda_a;
    p.use_er = (cfg.lambda_r0 > 0.0 && cfg.lambda_r1 > 0.0); p.use_es = (cfg.lambda_s0 > 0.0 && cfg.lambda_s1 > 0.0); p.use_ea = cfg.lambda_a > 0.0;
    p.fix_poses = cfg.fix_poses; p.fix_intr = cfg.fix_intrinsics; p.fix_dist = cfg.fix_distortion; p.fix_sdf = cfg.fix_sdf;
    return p;
}

constexpr int HALO_CAP = 1 << 20;      // (direction, peer, entry) items of a rank's halo plan

static int alloc_rows(i3d_context* c, int slots) {
    const size_t Acap = (size_t)c->N;
    ShardState& sd = c->shard;
    c->Acap = (int)Acap; c->slots = slots;
    CTX_HIP(c, c->obs_frame.alloc(Acap * slots)); CTX_HIP(c, c->obs_w.alloc(Acap * slots));
    { const size_t nrow = ((Acap + 63) / 64) * 64 * (size_t)slots;
      CTX_HIP(c, c->rows.alloc(nrow / 64 * ROW_BLOCK_F4)); CTX_HIP(c, c->row_wr.alloc(nrow)); }
    CTX_HIP(c, c->aflags.alloc(Acap)); CTX_HIP(c, c->nrows.alloc(Acap)); CTX_HIP(c, c->gmax.alloc(Acap / 64 + 2)); CTX_HIP(c, c->anbr.alloc(Acap * NUM_NBR));
    CTX_HIP(c, c->cull_bounds.alloc(Acap / 64 + 2)); CTX_HIP(c, c->cull_mask.alloc((Acap / 64 + 2) * (size_t)((c->K + 31) / 32)));
    CTX_HIP(c, c->regflags.alloc(Acap)); CTX_HIP(c, c->ea_free.alloc(Acap)); CTX_HIP(c, c->ea_w.alloc(Acap * 6));
    CTX_HIP(c, c->C.alloc(Acap * P_VOX)); CTX_HIP(c, c->treg.alloc(Acap * 8)); CTX_HIP(c, c->aux_part.alloc((size_t)AUX_PART_ROWS * aux_part_stride(c->K)));
    CTX_HIP(c, c->C2.alloc(Acap * P_VOX)); CTX_HIP(c, c->treg2.alloc(Acap * 8)); CTX_HIP(c, c->gc_part.alloc((size_t)GC_PART_ROWS * gc_part_stride(c->K)));
    { // sized for BOTH tile geometries: the 512-entry one needs the most slots on large grids (3 per entry; 1024: 2), but a grid of <= 512 entries is ONE
      // 1024-entry tile with 2048 halo slots against one 512-entry tile with 1536
      const size_t nt = (size_t)tile_plan_tiles_of((int)Acap, 512);
      const size_t nh = std::max(nt * (size_t)tile_plan_hmax_of(512), (size_t)tile_plan_tiles_of((int)Acap, 1024) * (size_t)tile_plan_hmax_of(1024));
      CTX_HIP(c, c->tp_lnbr.alloc(Acap * LNBR_WORDS)); CTX_HIP(c, c->tp_eaw.alloc(Acap * 6)); CTX_HIP(c, c->tp_halo_idx.alloc(nh)); CTX_HIP(c, c->tp_halo_cnt.alloc(nt)); CTX_HIP(c, c->tp_iota.alloc(nh));
      CTX_HIP(c, c->tp_ext_e.alloc(nh)); CTX_HIP(c, c->tp_ext_pos.alloc(nh)); CTX_HIP(c, c->tp_qh.alloc(2 * nh)); CTX_HIP(c, c->tp_overflow.alloc(1));
      CTX_HIP(c, c->tp_ext_off.alloc(Acap + (size_t)SHARD_ALIGN * ((c->comm ? c->comm->world : 1) + 1) + 8));      // chunk + 1 offsets (chunk >= A, a multiple of the slice alignment)
      CTX_HIP(c, c->cam_part.alloc((size_t)2048 * (((size_t)6 * c->K + 9 + 3) & ~(size_t)3)));                     // one float row of the camera block per operator workgroup
      CTX_HIP(c, c->tp_temp.alloc(tile_plan_temp_bytes(nt * (size_t)tile_plan_hmax_of(1024)))); }      // (>= the slots of either geometry's plan)
    const int world_a = c->comm ? c->comm->world : 1;
    const size_t NP = 2 * ((size_t)c->N + (size_t)SHARD_ALIGN * (world_a + 1)) + 6 * (size_t)c->K + 9;      // chunk = world * slice >= A, slice a multiple of SHARD_ALIGN
    for (DevBuf<float>* v : {&c->v_mask, &c->v_c, &c->v_S, &c->v_cm, &c->v_D2, &c->v_Minv, &c->v_b, &c->v_x, &c->v_r, &c->v_p, &c->v_z, &c->v_q, &c->v_u, &c->v_acc, &c->v_tmp, &c->v_qacc})
        { const bool fresh = v->n < NP || !v->p; CTX_HIP(c, v->alloc(NP)); if (fresh) CTX_HIP(c, hipMemsetAsync(v->p, 0, sizeof(float) * v->n, c->stream)); }   // padding entries stay finite (on the library's stream: it is non-blocking, a null-stream memset is not ordered against it)
    CTX_HIP(c, c->Minv_blocks.alloc((size_t)36 * c->K + 16 + 25));
    CTX_HIP(c, c->d_shared.alloc((size_t)6 * c->K + 9 + 1)); CTX_HIP(c, c->d_blocks.alloc((size_t)21 * c->K + 25));      // +1: p.q partial rides with the camera block
    CTX_HIP(c, sd.clist.alloc(Acap)); CTX_HIP(c, sd.cflag.alloc(Acap)); CTX_HIP(c, sd.cscan.alloc(Acap));
    if (c->comm) {      // sharding plan storage (small: the rim of a rank is a few percent of what it owns)
        const size_t cap = HALO_CAP;
        CTX_HIP(c, sd.need_mask.alloc(Acap)); CTX_HIP(c, sd.halo_items.alloc(cap)); CTX_HIP(c, sd.halo_sorted.alloc(cap)); CTX_HIP(c, sd.halo_count.alloc(1));
        CTX_HIP(c, sd.halo_send_idx.alloc(cap)); CTX_HIP(c, sd.halo_recv_idx.alloc(cap)); CTX_HIP(c, sd.halo_send_peer.alloc(cap)); CTX_HIP(c, sd.halo_recv_peer.alloc(cap)); CTX_HIP(c, sd.halo_offs.alloc(2 * P2P_MAX_RANKS)); CTX_HIP(c, sd.halo_send_buf.alloc((size_t)HALO_MULTI_MAX * (2 * cap))); CTX_HIP(c, sd.halo_recv_buf.alloc((size_t)HALO_MULTI_MAX * (2 * cap)));      /* a ladder batch pushes HALO_MULTI_MAX values per rim entry in one message */
        CTX_HIP(c, sd.halo_temp.alloc(halo_sort_temp_bytes((int)cap)));
        const size_t nt = (size_t)tile_plan_tiles_of((int)Acap, 512) + 1; CTX_HIP(c, sd.tile_flag.alloc(nt)); CTX_HIP(c, sd.ghost_tiles.alloc(nt));
    }
    CTX_HIP(c, c->d_scal.alloc(32)); CTX_HIP(c, c->d_xshared.alloc((size_t)6 * c->K + 9)); CTX_HIP(c, c->d_xcshared.alloc((size_t)6 * c->K + 9));
    CTX_HIP(c, c->d_pcg.alloc(1)); CTX_HIP(c, c->d_pcg2.alloc(2));
    CTX_HIP(c, c->d_partials.alloc((Acap / 256 + 2048) * 9));       // per-workgroup partial sums of the fp64 reductions
    if (!c->h_flags) { CTX_HIP(c, hipHostMalloc((void**)&c->h_flags, 32 * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));      // (pass, done) rings: 4 ints per system of a ladder batch
                       for (int i = 0; i < 32; ++i) c->h_flags[i] = -1;
                       CTX_HIP(c, hipHostGetDevicePointer((void**)&c->d_flags, c->h_flags, 0)); }
    CTX_HIP(c, c->d_lm.alloc(1)); CTX_HIP(c, c->d_cam_c.alloc((size_t)6 * c->K + 9)); CTX_HIP(c, c->d_cam_H.alloc((size_t)21 * c->K + 25));
    if (!c->h_lmrec) { CTX_HIP(c, hipHostMalloc((void**)&c->h_lmrec, LM_REC_SLOTS * sizeof(LmRecord), hipHostMallocMapped | hipHostMallocCoherent));
                       std::memset(c->h_lmrec, 0, LM_REC_SLOTS * sizeof(LmRecord));
                       CTX_HIP(c, hipHostGetDevicePointer((void**)&c->d_lmrec, c->h_lmrec, 0)); }
    for (auto& e : c->ev_asm) if (!e) CTX_HIP(c, hipEventCreate(&e));
    return ensure_pinned(c, 64 + (size_t)27 * c->K + 64);
}

// the sharding plan of this outer iteration: compute list, halo lists, ghost tiles — derived from the replicated work list, no communication
static int shard_plan(i3d_context* c) {
    hipStream_t s = c->stream;
    ShardState& sd = c->shard;
    const int world = c->comm->world, rank = c->comm->rank;
    if (world > 64) return ctx_fail(c, I3D_ERR_CAPACITY, "sharding: more than 64 ranks");
    shard_range(c->A, world, rank, sd.chunk, sd.own0, sd.own1); sd.nC = 0; sd.slice = sd.chunk / world;
    RowView r0 = c->row_view();
    TimedScope t(c, I3D_K_CLASSIFY);
    launch_mark_compute(s, r0, sd.cflag.p);
    CTX_HIP(c, rocprim::exclusive_scan(c->scan_tmp.p, c->scan_tmp_bytes, sd.cflag.p, sd.cscan.p, 0, (size_t)c->A, rocprim::plus<int>(), s));
    launch_compact_list(s, c->A, sd.cflag.p, sd.cscan.p, sd.clist.p);
    const int T = c->plan_T(), ntiles = tile_plan_tiles_of(c->A, T);
    CTX_HIP(c, hipMemsetAsync(sd.need_mask.p, 0, sizeof(unsigned long long) * (size_t)c->A, s));
    CTX_HIP(c, hipMemsetAsync(sd.halo_count.p, 0, sizeof(int), s));
    CTX_HIP(c, hipMemsetAsync(sd.tile_flag.p, 0, sizeof(int) * (size_t)(ntiles + 1), s));
    launch_need_mask(s, r0, sd.slice, sd.need_mask.p);
    launch_halo_items(s, c->A, sd.slice, rank, sd.need_mask.p, sd.halo_items.p, sd.halo_count.p, HALO_CAP);
    launch_tile_flags(s, c->A, T, sd.cflag.p, sd.tile_flag.p);
    int nitems = 0;
    ScanTotal listed; CTX_HIP(c, listed.queue(c, sd.cflag.p, sd.cscan.p, c->A));
    CTX_HIP(c, hipMemcpyAsync(&nitems, sd.halo_count.p, sizeof(int), hipMemcpyDeviceToHost, s));
    std::vector<int> tf((size_t)ntiles + 1, 0);
    CTX_HIP(c, hipMemcpyAsync(tf.data(), sd.tile_flag.p, sizeof(int) * (size_t)ntiles, hipMemcpyDeviceToHost, s));
    CTX_HIP(c, sync_stream(c));
    sd.nC = (int)listed.total();
    if (nitems > HALO_CAP) return ctx_fail(c, I3D_ERR_CAPACITY, "sharding: the halo plan does not fit its buffers");
    // ghost tiles: foreign tiles that hold compute-list entries
    std::vector<int> ghosts; const int t0 = sd.own0 / T, t1 = (sd.own1 + T - 1) / T;
    for (int i = 0; i < ntiles; ++i) if (tf[i] && (i < t0 || i >= t1)) ghosts.push_back(i);
    sd.n_ghost_tiles = (int)ghosts.size();
    if (!ghosts.empty()) CTX_HIP(c, hipMemcpyAsync(sd.ghost_tiles.p, ghosts.data(), sizeof(int) * ghosts.size(), hipMemcpyHostToDevice, s));
    // halo lists: items sorted by (direction, peer, entry) -> per-peer runs
    HaloPlan& h = sd.halo; h.world = world; h.chunk = sd.chunk;
    h.send_cnt.assign(world, 0); h.send_off.assign(world, 0); h.recv_cnt.assign(world, 0); h.recv_off.assign(world, 0); h.n_send = h.n_recv = 0;
    std::vector<unsigned long long> items((size_t)nitems);
    if (nitems > 0) {
        CTX_HIP(c, launch_halo_sort(s, sd.halo_temp.p, sd.halo_temp.n, sd.halo_items.p, sd.halo_sorted.p, nitems));
        CTX_HIP(c, hipMemcpyAsync(items.data(), sd.halo_sorted.p, sizeof(unsigned long long) * (size_t)nitems, hipMemcpyDeviceToHost, s));
        CTX_HIP(c, sync_stream(c));
    }
    std::vector<int> sidx, ridx, speer, rpeer;       // + the peer of every item: the flat lists the in-kernel exchanges of the three-launch pass walk (RimLists)
    for (unsigned long long it : items) {
        const int dir = (int)(it >> 40) & 1, peer = (int)((it >> 32) & 0xFF), e = (int)(it & 0xFFFFFFFFull);
        if (dir == 0) { if (h.send_cnt[peer]++ == 0) h.send_off[peer] = (int)sidx.size(); sidx.push_back(e); speer.push_back(peer); }
        else          { if (h.recv_cnt[peer]++ == 0) h.recv_off[peer] = (int)ridx.size(); ridx.push_back(e); rpeer.push_back(peer); }
    }
    h.n_send = (int)sidx.size(); h.n_recv = (int)ridx.size();
    if (h.n_send) { CTX_HIP(c, hipMemcpyAsync(sd.halo_send_idx.p, sidx.data(), sizeof(int) * sidx.size(), hipMemcpyHostToDevice, s));
                    CTX_HIP(c, hipMemcpyAsync(sd.halo_send_peer.p, speer.data(), sizeof(int) * speer.size(), hipMemcpyHostToDevice, s)); }
    if (h.n_recv) { CTX_HIP(c, hipMemcpyAsync(sd.halo_recv_idx.p, ridx.data(), sizeof(int) * ridx.size(), hipMemcpyHostToDevice, s));
                    CTX_HIP(c, hipMemcpyAsync(sd.halo_recv_peer.p, rpeer.data(), sizeof(int) * rpeer.size(), hipMemcpyHostToDevice, s)); }
    int offs[2 * P2P_MAX_RANKS] = {0};
    for (int k = 0; k < world; ++k) { offs[k] = h.send_off[k]; offs[P2P_MAX_RANKS + k] = h.recv_off[k]; }
    CTX_HIP(c, hipMemcpyAsync(sd.halo_offs.p, offs, sizeof(offs), hipMemcpyHostToDevice, s));
    CTX_HIP(c, sync_stream(c));                  // (the host vectors above go out of scope)
    h.d_send_idx = sd.halo_send_idx.p; h.d_recv_idx = sd.halo_recv_idx.p; h.d_send_buf = sd.halo_send_buf.p; h.d_recv_buf = sd.halo_recv_buf.p;
    { const int prc = c->comm->plan_changed(h, s);
      if (prc == 2) return ctx_fail(c, I3D_ERR_CAPACITY, "sharding: the rim of a rank pair exceeds the peer-to-peer mailbox");
      if (prc) return ctx_fail(c, I3D_ERR_COMM, "sharding: installing the halo lists of the peer-to-peer transport failed on a rank (HIP / copy error)"); }
    return I3D_OK;
}

// The operator plan of an outer iteration, before anything is planned or built on it.  comm: the communicator of a sharded run, null on one rank; A: the work
// list's entries; last_entries / last_rows: active entries and Eg rows of the previous outer iteration (0: none yet).
static OperatorPlan plan_operator(const SolverSwitches& sw, int slots, int K, Comm* comm, int A, long long last_entries, long long last_rows) {
    OperatorPlan op;
    const bool sharded = comm != nullptr;
    // Bit-reproducible operator pass (fixed-order sums inside the workgroups of k_eg_tile as well): the default on one rank, where the multi-system pass is fixed-order
    // by construction and only the lone-system passes pay for it (0.7 % of an iteration, profiles/r05_bench_deterministic.json); I3D_DETERMINISTIC=0 selects the
    // LDS-atomic pass.  A sharded run iterates serially through k_eg_tile (5 % there): opt-in with I3D_DETERMINISTIC=1.
    op.deterministic = sw.deterministic >= 0 ? sw.deterministic == 1 : !sharded;
    // the damping ladder (lm_solve): up to I3D_LADDER consecutive LM attempts solved together, one stream of the rows per group of <= 3 of them (tile_pass_mr.hip);
    // 1 = the serial trust-region loop.  Needs the single-rank tiled pass in its 512-entry geometry with pull lists and the shipped 5 observation slots.
    op.ladder_max = sw.ladder;
    if (slots != 5 || eg_tile_mr_max_systems(K) < 2) op.ladder_max = 1;
    // sharded (round 6): the ladder runs with the exchanges as launches of the transport (RCCL, the rank simulation): pcg_solve_ladder all-reduces the batch's sums in
    // one message per exchange.  Over the mailboxes (the in-kernel exchanges of the three-launch serial pass, I3D_TRANSPORT=p2p) the serial loop stays.
    // This probe runs BEFORE this iteration's shard_plan(): whether every rim fits its mailbox is still the previous outer iteration's answer.  A run that flips
    // between mailbox and transport rims therefore plans 512-entry tiles and then solves serially, or leaves the ladder out where it could have run; solve_route
    // (solver.cpp) probes again behind the plan, so the results are right and only the geometry is stale (ADVICE.md finding 3, kept as it is here).
    if (sharded) { P2PDev probe; if (comm->fused_exchange(&probe)) op.ladder_max = 1; }
    // I3D_EGT_MR1=1: the SERIAL loop streams its rows through k_eg_tile_mr<1> (the multi-system kernel with one system) instead of k_eg_tile — the control of the
    // ladder tests (same kernel family: a system solved alone vs in a batch, bit for bit) and an A/B switch
    op.mr1_serial = sw.egt_mr1 && !sharded && slots == 5 && eg_tile_mr_max_systems(K) >= 1;
    op.ladder_lists = op.ladder_max > 1 || op.mr1_serial;
    // halo sums of the operator pass pulled over plan lists instead of pushed with LDS atomics: always in the bit-reproducible mode, else on request
    op.halo_pull = op.deterministic || sw.halo_pull;
    if (!sharded) {
        // tile geometry: 1024-entry tiles (one workgroup of 16 waves per CU) unless the work list is row-poor — SURVEY.md 8(d)'s 4-voxel shell, real sequences with few
        // observations: a third of the entries own no Eg rows, their waves idle while the others stream, and two smaller workgroups per CU keep more row blocks in
        // flight (measured on --band 2: 0.43 -> 0.39 ms per pass; on the 5.0-rows workload 512-entry tiles are 2.5 % slower).  The density is last iteration's
        // (rows per entry are a property of the grid, not of the iteration); either geometry is the other's fallback when a tile's halo does not fit.
        if (sw.egt_tile == 0 && last_entries > 0 && (double)last_rows < 0.8 * (double)slots * (double)last_entries) op.tile_T = 512;
        if (op.ladder_lists) op.tile_T = 512;      // the multi-system pass exists in the 512-entry geometry (8 waves at 2 per SIMD: the column sums of 3 systems live in registers)
    } else {
        // First choice: 1024-entry tiles (2048 halo slots; a third fewer tile boundaries, one workgroup per CU) when a rank's share fills at least two rounds of
        // them, else 512-entry tiles (1536 halo slots, two workgroups per CU): a small share balances better over twice the tiles.  Every rank derives the choice
        // from the replicated work list.
        // (256-entry tiles for shares below two rounds were built and measured in round 4: the operator gains 2 us per pass, the halo fold loses more —
        // profiles/r04_share_tile_ab.json — removed.)
        op.tile_T = (op.ladder_max > 1) ? 512 : ((A / comm->world >= 2 * 256 * 1024) ? 1024 : 512);      // the multi-system pass exists in the 512-entry geometry
    }
    return op;
}

static int queue_tile_plan(i3d_context* c) {
    RowView r0 = c->row_view(); TimedScope t(c, I3D_K_CLASSIFY);
    CTX_HIP(c, launch_tile_plan(c->stream, r0, c->tile_plan(), c->plan_hmax_limit(), c->tp_temp.p, c->tp_temp.n));
    return I3D_OK;
}

// The overflow fall-backs of a plan whose halo does not fit a tile.  First the other geometry (the caller plans again) ...
static void plan_other_geometry(i3d_context* c) {
    const int other = c->plan_T() == 512 ? 1024 : 512;
    std::fprintf(stderr, "[i3d] %soperator pass: a %d-entry tile's halo does not fit, planning again with %d-entry tiles\n", c->sharded() ? "sharded " : "", c->plan_T(), other);
    c->op.tile_T = other;
}
// ... then, with the overflow flag of the last plan: on one rank the untiled pass (pathological grids), sharded an error (a sharded run has no untiled pass)
static int settle_plan(i3d_context* c, int tp_over) {
    c->op.tile_ok = tp_over == 0;
    if (c->sharded()) return c->op.tile_ok ? I3D_OK : ctx_fail(c, I3D_ERR_CAPACITY, "sharded optimize: the tile plan overflowed after it had been accepted");      // (cannot happen: agreed on in assemble)
    if (!c->op.tile_ok) std::fprintf(stderr, "[i3d] operator pass: a tile's halo does not fit, using the untiled pass (k_eg_jtjp + k_gather)\n");
    if (c->sw.no_tile) c->op.tile_ok = false;      // tests of the single-rank fallback (k_eg_jtjp + k_gather)
    return I3D_OK;
}

int assemble(i3d_context* c, const i3d_optimizer_config& cfg, int iteration, OptParams& p, i3d_iteration_stats* st) {
    read_switches(c);
    const SolverSwitches& sw = c->sw;
    ShardState& sd = c->shard;
    if (!c->have_grid || !c->have_frames || !c->have_camera) return ctx_fail(c, I3D_ERR_STATE, "optimize: grid, keyframes and camera must be set");
    if (cfg.rgbd_level < 0 || cfg.rgbd_level >= c->levels) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "optimize: rgbd_level outside the uploaded pyramid");
    int slots = (cfg.num_observations <= 0 || cfg.num_observations >= c->K) ? c->K : cfg.num_observations;
    if (slots > MAX_SLOTS) return ctx_fail(c, I3D_ERR_CAPACITY, "optimize: more than 8 observations per voxel requested");
    if (c->K > 2000) return ctx_fail(c, I3D_ERR_CAPACITY, "optimize: more than 2000 keyframes (the camera accumulators of the operator pass live in 160 KB of LDS)");
    if (c->slots != slots || c->Acap != c->N || !c->rows.p) { int rc = alloc_rows(c, slots); if (rc) return rc; }
    hipStream_t s = c->stream;
    CTX_HIP(c, hipEventRecord(c->ev_asm[0], s));
    p = make_params(c, cfg);
    GridView g = c->grid_view();
    { TimedScope t(c, I3D_K_CLASSIFY);
      launch_classify(s, g, p, c->aflag.p);
      CTX_HIP(c, rocprim::exclusive_scan(c->scan_tmp.p, c->scan_tmp_bytes, c->aflag.p, c->ascan.p, 0, (size_t)c->N, rocprim::plus<int>(), s));
      launch_compact(s, c->N, c->aflag.p, c->ascan.p, c->flags.p, c->aidx.p, c->alist.p, c->aflags.p); }
    int tail[2];
    CTX_HIP(c, hipMemcpyAsync(&tail[0], c->ascan.p + (c->N - 1), sizeof(int), hipMemcpyDeviceToHost, s));
    CTX_HIP(c, hipMemcpyAsync(&tail[1], c->aflag.p + (c->N - 1), sizeof(int), hipMemcpyDeviceToHost, s));
    // the keyframe constants of this iteration's poses (host, fp64, the reference's libm) while the device classifies: the host would wait here anyway
    std::vector<FrameConst> fc; build_frame_consts(c, cfg.rgbd_level, c->poses.data(), fc);
    CTX_HIP(c, sync_stream(c));
    CTX_HIP(c, hipMemcpyAsync(c->d_frames.p, fc.data(), sizeof(FrameConst) * fc.size(), hipMemcpyHostToDevice, s));
    c->A = tail[0] + tail[1];
    { TimedScope t(c, I3D_K_CLASSIFY);
      launch_partition_blocks(s, g, c->A, c->alist.p, c->aflags.p, c->aidx.p);
      launch_anbr(s, c->N, c->A, c->Acap, c->alist.p, c->nbr.p, c->aidx.p, c->anbr.p); }
    c->op = plan_operator(sw, slots, c->K, c->sharded() ? c->comm : nullptr, c->A, c->last_sizes[0], c->last_sizes[1]);
    if (c->op.pull_lists()) {      // sized for both tile geometries (Acap entries)
        const size_t n512 = (size_t)tile_plan_tiles_of(c->Acap, 512), n1024 = (size_t)tile_plan_tiles_of(c->Acap, 1024);
        CTX_HIP(c, c->tp_hp_off.alloc(std::max(n512 * (size_t)(1536 + 1), n1024 * (size_t)(2048 + 1)) + 8));
        CTX_HIP(c, c->tp_hp_src.alloc(std::max(n512 * (size_t)tile_plan_pull_cap(1536), n1024 * (size_t)tile_plan_pull_cap(2048)) + 8));
    }
    if (!c->sharded()) {
        shard_range(c->A, 1, 0, sd.chunk, sd.own0, sd.own1); sd.nC = c->A; sd.slice = sd.chunk;
        { int rc = queue_tile_plan(c); if (rc) return rc; }
    } else {
        // owned range + compute list + halo lists + ghost tiles (every rank derives them from the replicated work list: no communication), then the tile plan.
        // A sharded run has no untiled operator: when a tile's halo does not fit anywhere (the ranks agree: max over ranks), all of them plan again with the
        // other geometry before anything is built on the plan.
        for (int attempt = 0; attempt < 2; ++attempt) {
            int rc = shard_plan(c); if (rc) return rc;
            rc = queue_tile_plan(c); if (rc) return rc;
            launch_fill_d(s, 1, c->d_scal.p + 20, 0.0); launch_int_to_double(s, c->tp_overflow.p, c->d_scal.p + 20);
            rc = allreduce(c, c->d_scal.p + 20, 1); if (rc) return rc;
            double over = 0.0; rc = read_doubles(c, c->d_scal.p + 20, 1, &over); if (rc) return rc;
            if (over == 0.0) break;
            if (attempt == 1) return ctx_fail(c, I3D_ERR_CAPACITY, "sharded optimize: a tile of the operator pass reaches more foreign entries than either tile geometry has halo slots");
            plan_other_geometry(c);
        }
        // rows are only built on the compute list: everything else on the tiles this rank runs must be inert
        CTX_HIP(c, hipMemsetAsync(c->nrows.p, 0, (size_t)c->A, s)); CTX_HIP(c, hipMemsetAsync(c->regflags.p, 0, (size_t)c->A, s));
    }
    RowView r = c->row_view();
    { TimedScope t(c, I3D_K_OBSERVE);
      // conservative (group of 64 entries, keyframe) culling: the depth-range pyramid once per keyframe set and level, spheres and masks per iteration
      // I3D_NO_CULL (A/B runs and the with / without test): 1 = neither, 2 = no group masks, 3 = no weight-bound prefilter
      const int mode = sw.no_cull;
      const unsigned* mask = nullptr; c->cull_on = !(mode == 1 || mode == 2); const bool prefilter = !(mode == 1 || mode == 3);
      if (c->cull_on) {
          if (c->cull_level != cfg.rgbd_level || !c->cull_blocks.p) {
              CTX_HIP(c, c->cull_blocks.alloc((size_t)c->K * cull_pyramid(p.w, p.h).cells));
              launch_depth_blocks(s, c->d_frames.p, c->K, p.w, p.h, c->cull_blocks.p); c->cull_level = cfg.rgbd_level; }
          launch_group_cull(s, g, r, p, c->d_frames.p, c->cull_blocks.p, c->cull_bounds.p, c->cull_mask.p); mask = c->cull_mask.p; }
      launch_observe(s, g, r, p, c->d_frames.p, mask, prefilter); }
    // the reference's three-way split (nls_solver.cpp:66-67,101): time_add = collecting the residuals (addVoxelResiduals: classification, observations),
    // time_build = buildProblem (cost functions, weight normalisation), time_solve.  The boundary is an event on the stream (round 3: a synchronisation).
    CTX_HIP(c, hipEventRecord(c->ev_asm[1], s));
    { TimedScope t(c, I3D_K_BUILD); launch_build(s, g, r, p, c->d_frames.p, true, nullptr, c->d_partials.p); }
    { TimedScope t(c, I3D_K_CLASSIFY); launch_group_rows(s, c->A, c->nrows.p, c->gmax.p); }
    { TimedScope t(c, I3D_K_CLASSIFY); launch_eaw_sym(s, r, c->tile_plan(), c->sharded() ? sd.cflag.p : nullptr); }
    CTX_HIP(c, hipMemsetAsync(c->d_scal.p, 0, sizeof(double) * 32, s));
    { TimedScope t(c, I3D_K_VECTOR); launch_weight_sums(s, r, g, cost_from_sums(c), c->d_scal.p, c->d_partials.p); }
    { int rc = allreduce(c, c->d_scal.p, 13); if (rc) return rc; }
    int tp_over = 1;
    CTX_HIP(c, hipMemcpyAsync(&tp_over, c->tp_overflow.p, sizeof(int), hipMemcpyDeviceToHost, s));
    double sums[13]; { int rc = read_doubles(c, c->d_scal.p, 13, sums); if (rc) return rc; }
    if (c->sharded() && c->comm->health(s)) return ctx_fail(c, I3D_ERR_COMM, "assemble: a peer-to-peer exchange timed out (a rank stopped taking part)");
    if (!c->sharded() && tp_over != 0) {      // single rank: the other geometry before giving up on the tiled pass (the symmetric Ea weights do not depend on the geometry)
        plan_other_geometry(c);
        { int rc = queue_tile_plan(c); if (rc) return rc; }
        CTX_HIP(c, hipMemcpyAsync(&tp_over, c->tp_overflow.p, sizeof(int), hipMemcpyDeviceToHost, s));
        CTX_HIP(c, sync_stream(c));
    }
    { int rc = settle_plan(c, tp_over); if (rc) return rc; }
    sums[5] = sums[1]; sums[6] = sums[2];
    const double lambda[4] = {cfg.lambda_g, varying_lambda(iteration, cfg.iterations, cfg.lambda_r0, cfg.lambda_r1),
                              varying_lambda(iteration, cfg.iterations, cfg.lambda_s0, cfg.lambda_s1), cfg.lambda_a};
    for (int t = 0; t < 4; ++t) { p.type_w[t] = sums[t] != 0.0 ? (lambda[t] / sums[t]) * 1000.0 : 0.0; p.type_wf[t] = (float)p.type_w[t]; }     // nls_solver.cpp:379-394
    c->n_active = (long long)(sums[8] + 0.5);
    // the cost at the point the rows were built at (k_weight_sums): what the trust-region loop starts from
    c->cost_at_build = 0.5 * (p.type_w[0] * sums[9] + p.type_w[1] * sums[10] + p.type_w[2] * sums[11] + p.type_w[3] * sums[12]);
    if (st) { for (int t = 0; t < 4; ++t) { st->rows[t] = (int64_t)(sums[4 + t] + 0.5); st->weight_sum[t] = sums[t]; st->type_weight[t] = p.type_w[t]; } st->valid_voxels = c->n_active; }
    c->last_sizes[0] = c->n_active; for (int t = 0; t < 4; ++t) c->last_sizes[1 + t] = (long long)(sums[4 + t] + 0.5);
    c->last_params = p; c->assembled = true;
    { float ms = 0.0f; c->t_add_end = (hipEventElapsedTime(&ms, c->ev_asm[0], c->ev_asm[1]) == hipSuccess) ? (double)ms * 1e-3 : -1.0; }      // (both events lie before the read-back above)
    { const int lrc = ctx_launch_check(c); if (lrc) return lrc; }
    return I3D_OK;
}

}  // namespace i3d
