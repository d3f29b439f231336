// i3d_debug_lm_script (tests only): the controller kernels of the trust-region loop (lm_kernels.hip: k_lm_init, k_lm_begin, k_lm_begin_lad, k_lm_decide) run ALONE,
// through the launch_* functions lm_solve uses and in the order it queues them (solver.cpp), on a script of attempt outcomes the caller supplies: what the PCG solve,
// the candidate kernel and the cost pass would have left on the device.  No grid, no rows; buffers of its own; the context's solver state is not touched.
//   serial loop (empty plan)   k_lm_begin(k) | record k-1 read | k_lm_decide(k, lad_next = -1)
//   ladder (batch plan)        k_lm_begin_lad(B) | k_lm_decide(k + j, lad_next = j + 1), j = 0 .. B-1, all queued | records read; a kind-3 record: its slot is cleared and
//                              attempt k + j starts a batch of one
// Every begin writes its block-Jacobi inverses, LM diagonal and (serial loop) 1x1 inverses into a slot of its own, with I3D_LM_SCRIPT_GUARD floats of NaN on either
// side; a slot no kernel wrote stays NaN.
#include <cstring>
#include <vector>
#include "context.hpp"

using namespace i3d;

namespace {
constexpr int G = I3D_LM_SCRIPT_GUARD;
constexpr int REC_SLOTS = 64;          // as lm_solve's ring: the initial tests + one record per attempt + the look-ahead record of the last one
}

extern "C" int i3d_debug_lm_script(i3d_context* c, const i3d_lm_script_desc* d, i3d_lm_record* records, int32_t* n_records, double* state25, int32_t* n_setups,
                                   int32_t* setup_meta, double* setup_radius, float* setup_inv_radius, float* setup_blocks, float* setup_d2, float* setup_minv) {
    const char* fn = "i3d_debug_lm_script";
    if (!c) return I3D_ERR_INVALID_ARGUMENT;
    if (!d || !records || !n_records || !state25 || !n_setups || !setup_meta || !setup_radius || !setup_inv_radius || !setup_blocks || !setup_d2 || !setup_minv)
        return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null argument");
    if (d->lm_steps < 1 || d->lm_steps > REC_SLOTS - 2) return ctx_fail(c, I3D_ERR_CAPACITY, std::string(fn) + ": lm_steps must be 1..62 (the record ring)");
    if (d->n_attempts < d->lm_steps) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": fewer scripted attempts than lm_steps");
    if (d->K < 0 || d->K > 4096 || d->n_plan < 0 || d->max_setups < 1) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": K, n_plan or max_setups out of range");
    if (!d->cdiag || !d->tri || !d->tail_c || !d->tail_S || !d->xbr || !d->d2xx || !d->pcg_it || !d->pcg_done || !d->norms2 || !d->cand_cost || !d->debug_invalid || (d->n_plan > 0 && !d->plan))
        return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": null array in the script");
    for (int i = 0; i < d->n_plan; ++i) if (d->plan[i] < 1 || d->plan[i] > LADDER_MAX) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, std::string(fn) + ": batch sizes must be 1..LADDER_MAX");
    static_assert(sizeof(i3d_lm_record) == sizeof(LmRecord), "i3d_lm_record mirrors LmRecord");

    CTX_HIP(c, hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int K = d->K, NS = 6 * K + 9, NB = 36 * K + 41, NT = 21 * K + 25, n = d->n_attempts, S = d->max_setups;
    const size_t WB = (size_t)NB + 2 * G, WT = (size_t)NS + 2 * G;          // slot widths: guard | output | guard

    DevBuf<LmState> lm, snaps; DevBuf<LmRecord> rec; DevBuf<PcgState> ps; DevBuf<double> dbl; DevBuf<float> tail, blocks, d2, minv;
    CTX_HIP(c, lm.alloc(1)); CTX_HIP(c, snaps.alloc((size_t)S)); CTX_HIP(c, rec.alloc(REC_SLOTS)); CTX_HIP(c, ps.alloc((size_t)n));
    CTX_HIP(c, dbl.alloc(3 + (size_t)NS + NT + 3 * (size_t)n)); CTX_HIP(c, tail.alloc(2 * (size_t)NS));
    CTX_HIP(c, blocks.alloc(WB * S)); CTX_HIP(c, d2.alloc(WT * S)); CTX_HIP(c, minv.alloc(WT * S));
    // the script, uploaded once: [cost ngrad nfree | cdiag | tri | norms2 | cand_cost]
    std::vector<double> hd(dbl.n);
    hd[0] = d->cost; hd[1] = d->ngrad; hd[2] = d->nfree;
    std::memcpy(hd.data() + 3, d->cdiag, sizeof(double) * NS); std::memcpy(hd.data() + 3 + NS, d->tri, sizeof(double) * NT);
    std::memcpy(hd.data() + 3 + NS + NT, d->norms2, sizeof(double) * 2 * n); std::memcpy(hd.data() + 3 + NS + NT + 2 * (size_t)n, d->cand_cost, sizeof(double) * n);
    std::vector<PcgState> hps((size_t)n);
    std::memset(hps.data(), 0, sizeof(PcgState) * hps.size());
    for (int i = 0; i < n; ++i) { hps[i].xbr = d->xbr[i]; hps[i].d2xx = d->d2xx[i]; hps[i].it = d->pcg_it[i]; hps[i].done = d->pcg_done[i]; hps[i].fixed_iterations = -1; hps[i].max_iterations = 500; }
    std::vector<float> ht(2 * (size_t)NS);
    std::memcpy(ht.data(), d->tail_c, sizeof(float) * NS); std::memcpy(ht.data() + NS, d->tail_S, sizeof(float) * NS);
    CTX_HIP(c, hipMemcpyAsync(dbl.p, hd.data(), sizeof(double) * hd.size(), hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(ps.p, hps.data(), sizeof(PcgState) * hps.size(), hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(tail.p, ht.data(), sizeof(float) * ht.size(), hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemsetAsync(rec.p, 0, sizeof(LmRecord) * REC_SLOTS, s));
    CTX_HIP(c, hipMemsetAsync(snaps.p, 0, sizeof(LmState) * (size_t)S, s));
    CTX_HIP(c, hipMemsetAsync(blocks.p, 0xFF, sizeof(float) * WB * S, s));      // 0xFFFFFFFF: a NaN
    CTX_HIP(c, hipMemsetAsync(d2.p, 0xFF, sizeof(float) * WT * S, s));
    CTX_HIP(c, hipMemsetAsync(minv.p, 0xFF, sizeof(float) * WT * S, s));
    const double* const cdiag = dbl.p + 3; const double* const tri = cdiag + NS; const double* const norms2 = tri + NT; const double* const cand = norms2 + 2 * (size_t)n;
    const float* const tc = tail.p; const float* const tS = tail.p + NS;

    const int seq0 = 1;
    int nrec = 0, nset = 0; bool ended = false;
    LmRecord h;
    // record `idx` of the solve, after everything queued so far (lm_solve polls mapped memory instead)
    auto read_record = [&](int idx, int seq) -> int {
        CTX_HIP(c, hipMemcpyAsync(&h, rec.p + idx, sizeof(LmRecord), hipMemcpyDeviceToHost, s));
        CTX_HIP(c, hipStreamSynchronize(s));
        if (h.seq != seq) return ctx_fail(c, I3D_ERR_STATE, std::string(fn) + ": record " + std::to_string(idx) + " was not published");
        return I3D_OK;
    };
    auto push = [&]() { std::memcpy(&records[nrec++], &h, sizeof(LmRecord)); if (h.final_) ended = true; };
    auto meta = [&](int slot, int attempt, int j, int B) { setup_meta[4 * slot] = attempt; setup_meta[4 * slot + 1] = j; setup_meta[4 * slot + 2] = B; setup_meta[4 * slot + 3] = 0; };

    launch_lm_init(s, lm.p, dbl.p, dbl.p + 1, dbl.p + 2, d->radius0, rec.p, seq0);
    int rc = I3D_OK;
    if (d->n_plan > 0) {
        rc = read_record(0, seq0); if (rc) return rc;
        push();
        int k = 0, pi = 0; bool after_resync = false;
        while (k < d->lm_steps && !ended) {
            int B = after_resync ? 1 : d->plan[pi < d->n_plan ? pi++ : d->n_plan - 1];
            B = std::max(1, std::min(B, std::min((int)LADDER_MAX, d->lm_steps - k)));
            after_resync = false;
            if (nset + B > S) return ctx_fail(c, I3D_ERR_CAPACITY, std::string(fn) + ": more begins than max_setups");
            launch_lm_begin_lad(s, lm.p, B, K, d->fix_poses, d->fix_intr, d->fix_dist, cdiag, tri, blocks.p + WB * nset + G, WB, tc, tS, d2.p + WT * nset + G, WT, rec.p + 1 + k, seq0 + 1 + k);
            CTX_HIP(c, hipMemcpyAsync(snaps.p + nset, lm.p, sizeof(LmState), hipMemcpyDeviceToDevice, s));
            for (int j = 0; j < B; ++j) meta(nset + j, k + j, j, B);
            nset += B;
            for (int j = 0; j < B; ++j)
                launch_lm_decide(s, lm.p, ps.p + k + j, norms2 + 2 * (size_t)(k + j), cand + k + j, k + j, d->lm_steps, rec.p + 1 + k + j, seq0 + 1 + k + j, j + 1, d->debug_invalid[k + j] ? 1 : 0);
            int decided = 0;
            for (int j = 0; j < B && !ended; ++j) {
                rc = read_record(1 + k + j, seq0 + 1 + k + j); if (rc) return rc;
                if (nrec >= 2 * REC_SLOTS) return ctx_fail(c, I3D_ERR_CAPACITY, std::string(fn) + ": more than 128 records");
                if (h.kind == 3) {
                    push();
                    CTX_HIP(c, hipMemsetAsync(rec.p + 1 + k + j, 0, sizeof(LmRecord), s));
                    after_resync = true; break;
                }
                push(); ++decided;
            }
            k += decided;
        }
    } else {
        int k = 0;
        for (; k < d->lm_steps; ++k) {
            if (nset + 1 > S) return ctx_fail(c, I3D_ERR_CAPACITY, std::string(fn) + ": more begins than max_setups");
            launch_lm_begin(s, lm.p, K, d->fix_poses, d->fix_intr, d->fix_dist, cdiag, tri, blocks.p + WB * nset + G, tc, tS, d2.p + WT * nset + G, minv.p + WT * nset + G, rec.p + 1 + k, seq0 + 1 + k);
            CTX_HIP(c, hipMemcpyAsync(snaps.p + nset, lm.p, sizeof(LmState), hipMemcpyDeviceToDevice, s));
            meta(nset, k, 0, 0); ++nset;
            rc = read_record(k, seq0 + k); if (rc) return rc;
            push();
            if (ended) break;
            launch_lm_decide(s, lm.p, ps.p + k, norms2 + 2 * (size_t)k, cand + k, k, d->lm_steps, rec.p + 1 + k, seq0 + 1 + k, -1, d->debug_invalid[k] ? 1 : 0);
        }
        if (!ended) { rc = read_record(k, seq0 + k); if (rc) return rc; push(); }
    }
    *n_records = nrec; *n_setups = nset;

    LmState fin; std::vector<LmState> hs((size_t)std::max(nset, 1));
    CTX_HIP(c, hipMemcpyAsync(&fin, lm.p, sizeof(LmState), hipMemcpyDeviceToHost, s));
    CTX_HIP(c, hipMemcpyAsync(hs.data(), snaps.p, sizeof(LmState) * hs.size(), hipMemcpyDeviceToHost, s));
    CTX_HIP(c, hipMemcpyAsync(setup_blocks, blocks.p, sizeof(float) * WB * nset, hipMemcpyDeviceToHost, s));
    CTX_HIP(c, hipMemcpyAsync(setup_d2, d2.p, sizeof(float) * WT * nset, hipMemcpyDeviceToHost, s));
    CTX_HIP(c, hipMemcpyAsync(setup_minv, minv.p, sizeof(float) * WT * nset, hipMemcpyDeviceToHost, s));
    CTX_HIP(c, hipStreamSynchronize(s));
    for (int i = 0; i < nset; ++i) {
        const int j = setup_meta[4 * i + 1], B = setup_meta[4 * i + 2];
        const LmState& st = hs[(size_t)(i - j)];                                   // the snapshot taken behind the begin kernel of this slot's batch
        setup_meta[4 * i + 3] = st.done;                                           // LmState::done behind the begin kernel
        setup_radius[i] = B > 0 ? st.lad_radius[j] : st.radius;
        setup_inv_radius[i] = B > 0 ? st.lad_inv_radius[j] : st.inv_radius;
    }
    double* o = state25;
    o[0] = fin.cost; o[1] = fin.radius; o[2] = fin.decrease_factor; o[3] = fin.ngrad; o[4] = fin.nfree; o[5] = fin.inv_radius;
    o[6] = fin.done; o[7] = fin.termination; o[8] = fin.accepted; o[9] = fin.invalid; o[10] = fin.attempts; o[11] = fin.successful; o[12] = fin.lad_n;
    for (int j = 0; j < LADDER_MAX; ++j) { o[13 + j] = fin.lad_radius[j]; o[13 + LADDER_MAX + j] = fin.lad_inv_radius[j]; }
    return ctx_launch_check(c);
}
