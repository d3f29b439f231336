// Readbacks of the assembled solver state, handed out in the caller's visit order (VisitOrder, context.hpp): the classification flags and the neighbour table of
// the grid, the Eg and regulariser rows of the last i3d_debug_assemble, the culling masks, and the parity probes of the normal equations
// (i3d_debug_normal_eq / _jtj_apply / _work_list): the passes of pcg.cpp on those rows.
#include "solver_internal.hpp"

using namespace i3d;

extern "C" {

int i3d_debug_flags(i3d_context* c, uint8_t* flags) {
    CTX_ENTER(c, flags && c->have_grid, ctx_fail(c, I3D_ERR_STATE, "i3d_debug_flags: no grid"));
    const int N = c->N; std::vector<uint8_t> f(N); VisitOrder vo;
    CTX_HIP(c, ctx_download(c, f.data(), c->flags.p, f.size()));
    if (int rc = vo.fetch(c, false)) return rc;
    CTX_HIP(c, ctx_sync(c));
    for (int s = 0; s < N; ++s) flags[vo.rank[s]] = f[s];
    return I3D_OK;
}

int i3d_debug_neighbors(i3d_context* c, int32_t* nbr) {
    CTX_ENTER(c, nbr && c->have_grid, ctx_fail(c, I3D_ERR_STATE, "i3d_debug_neighbors: no grid"));
    const int N = c->N; std::vector<int> t((size_t)NUM_NBR * N); VisitOrder vo;
    CTX_HIP(c, ctx_download(c, t.data(), c->nbr.p, t.size()));
    if (int rc = vo.fetch(c, false)) return rc;
    CTX_HIP(c, ctx_sync(c));
    for (int s = 0; s < N; ++s) for (int i = 0; i < NUM_NBR; ++i) { const int n = t[(size_t)i * N + s]; nbr[(size_t)vo.rank[s] * NUM_NBR + i] = n < 0 ? -1 : vo.rank[n]; }
    return I3D_OK;
}

int i3d_debug_eg_rows(i3d_context* c, int32_t* frame, float* weight, float* residual, float* jac) {
    CTX_ENTER(c, c->assembled, ctx_fail(c, I3D_ERR_STATE, "i3d_debug_eg_rows: not assembled"));
    const int N = c->N, A = c->A, S = c->slots; const size_t Acap = c->Acap;
    const size_t nrow = ((Acap + 63) / 64) * 64 * (size_t)S;
    VisitOrder vo; std::vector<float4> rows(nrow / 64 * ROW_BLOCK_F4); std::vector<float2> wr(nrow); std::vector<uint8_t> nr(Acap), afl(Acap);
    if (int rc = vo.fetch(c, true)) return rc;
    CTX_HIP(c, ctx_download(c, rows.data(), c->rows.p, rows.size()));
    CTX_HIP(c, ctx_download(c, wr.data(), c->row_wr.p, wr.size()));
    CTX_HIP(c, ctx_download(c, nr.data(), c->nrows.p, nr.size()));
    CTX_HIP(c, ctx_download(c, afl.data(), c->aflags.p, afl.size()));
    CTX_HIP(c, ctx_sync(c));
    const float2* const jt = reinterpret_cast<const float2*>(rows.data());
    for (size_t i = 0; i < (size_t)N * S; ++i) { if (frame) frame[i] = -1; if (weight) weight[i] = 0.0f; if (residual) residual[i] = 0.0f; }
    if (jac) std::memset(jac, 0, sizeof(float) * (size_t)N * S * P_TOTAL);
    const float tw = (float)c->last_params.type_w[0];
    for (int a = 0; a < A; ++a) {
        if (!(afl[a] & F_ACTIVE)) continue;
        const int v = vo.of_entry(a);
        for (int k = 0; k < (int)nr[a]; ++k) {
            const float2 m = wr[row_scalar_index(a, k, S)];
            if (m.x == 0.0f) continue;
            const size_t o = (size_t)v * S + k;
            if (frame) { int f; std::memcpy(&f, &jt[row_jt_index(a, k, S)].y, sizeof(int)); frame[o] = f & ~ROW_FREE_BIT; }
            if (weight) weight[o] = m.x * tw;
            if (residual) residual[o] = m.y;
            if (jac) {      // stored with the row weight folded in (Js = sqrt(w) J): handed out as the raw partials
                const float isw = 1.0f / std::sqrt(m.x);
                for (int q = 0; q < 7; ++q) { const float4 t = rows[row_index(a, k, q, S)]; jac[o * P_TOTAL + 4 * q] = t.x * isw; jac[o * P_TOTAL + 4 * q + 1] = t.y * isw; jac[o * P_TOTAL + 4 * q + 2] = t.z * isw; jac[o * P_TOTAL + 4 * q + 3] = t.w * isw; }
                jac[o * P_TOTAL + 28] = jt[row_jt_index(a, k, S)].x * isw;
            }
        }
    }
    return I3D_OK;
}

int i3d_debug_reg_rows(i3d_context* c, uint8_t* has_er, uint8_t* has_es, float* ea_weight) {
    CTX_ENTER(c, c->assembled, ctx_fail(c, I3D_ERR_STATE, "i3d_debug_reg_rows: not assembled"));
    const int N = c->N, A = c->A; const size_t Acap = c->Acap;
    VisitOrder vo; std::vector<uint8_t> rf(Acap), afl(Acap); std::vector<float> ew(Acap * 6);
    if (int rc = vo.fetch(c, true)) return rc;
    CTX_HIP(c, ctx_download(c, rf.data(), c->regflags.p, rf.size()));
    CTX_HIP(c, ctx_download(c, afl.data(), c->aflags.p, afl.size()));
    CTX_HIP(c, ctx_download(c, ew.data(), c->ea_w.p, ew.size()));
    CTX_HIP(c, ctx_sync(c));
    for (int v = 0; v < N; ++v) { if (has_er) has_er[v] = 0; if (has_es) has_es[v] = 0; if (ea_weight) for (int d = 0; d < 6; ++d) ea_weight[(size_t)v * 6 + d] = 0.0f; }
    const float tw = (float)c->last_params.type_w[3];
    for (int a = 0; a < A; ++a) {
        if (!(afl[a] & F_ACTIVE)) continue;
        const int v = vo.of_entry(a);
        if (has_er) has_er[v] = rf[a] & 1;
        if (has_es) has_es[v] = (rf[a] >> 1) & 1;
        if (ea_weight) for (int d = 0; d < 6; ++d) ea_weight[(size_t)v * 6 + d] = ew[(size_t)d * Acap + a] * tw;
    }
    return I3D_OK;
}

int i3d_debug_cull_stats(i3d_context* c, int64_t* pairs, int64_t* culled) {
    CTX_ENTER(c, pairs && culled, I3D_ERR_INVALID_ARGUMENT);
    if (!c->cull_mask.p || c->shard.nC <= 0) return ctx_fail(c, I3D_ERR_STATE, "i3d_debug_cull_stats: nothing assembled");
    const size_t ngroups = ((size_t)c->shard.nC + 63) / 64, ncw = ((size_t)c->K + 31) / 32;
    *pairs = (int64_t)(ngroups * (size_t)c->K);
    if (!c->cull_on) { *culled = -1; return I3D_OK; }
    std::vector<unsigned> m(ngroups * ncw);
    CTX_HIP(c, ctx_download(c, m.data(), c->cull_mask.p, m.size()));
    CTX_HIP(c, ctx_sync(c));
    int64_t n = 0; for (unsigned w : m) n += __builtin_popcount(w);
    *culled = n;
    return I3D_OK;
}

int i3d_debug_normal_eq(i3d_context* c, double* gradient, double* jtj_diag, double* cost) {
    CTX_ENTER(c, true, I3D_ERR_INVALID_ARGUMENT);
    if (!c->assembled) return ctx_fail(c, I3D_ERR_STATE, "debug: call i3d_debug_assemble first");
    OptParams p = c->last_params;
    VisitOrder vo; int rc = vo.fetch(c, true); if (rc) return rc;
    launch_freemask(c->stream, c->row_view(), p, c->v_mask.p);
    if (jtj_diag) { rc = run_pass(c, PASS_COLNORM, p, nullptr, c->v_c.p); if (rc) return rc; CTX_HIP(c, sync_stream(c)); rc = vo.vector_to_visit(c, c->v_c.p, jtj_diag); if (rc) return rc; }
    if (gradient) { rc = run_pass(c, PASS_GRAD, p, nullptr, c->v_acc.p); if (rc) return rc; CTX_HIP(c, sync_stream(c)); rc = vo.vector_to_visit(c, c->v_acc.p, gradient); if (rc) return rc; }
    if (cost) {
        rc = eval_cost_launch(c, p, false, c->d_frames.p); if (rc) return rc;
        rc = read_doubles(c, c->d_scal.p + 16, 1, cost); if (rc) return rc;
        if (c->sharded() && c->comm->health(c->stream)) return ctx_fail(c, I3D_ERR_COMM, "cost evaluation: a peer-to-peer exchange timed out (a rank stopped taking part)");
    }
    return I3D_OK;
}

int i3d_debug_jtj_apply(i3d_context* c, const double* x, double* y) {
    CTX_ENTER(c, x && y, ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_debug_jtj_apply: null pointer"));
    if (!c->assembled) return ctx_fail(c, I3D_ERR_STATE, "debug: call i3d_debug_assemble first");
    const int N = c->N, A = c->A, K = c->K, NS = 6 * K + 9, ch = c->shard.chunk, NP = 2 * ch + NS;
    OptParams p = c->last_params;
    VisitOrder vo; std::vector<float> h(NP, 0.0f), m(NP);
    int rc = vo.fetch(c, true); if (rc) return rc;
    launch_freemask(c->stream, c->row_view(), p, c->v_mask.p);
    CTX_HIP(c, ctx_download(c, m.data(), c->v_mask.p, m.size()));
    CTX_HIP(c, sync_stream(c));
    for (int a = 0; a < A; ++a) { const int v = vo.of_entry(a); h[a] = (float)x[v] * m[a]; h[ch + a] = (float)x[N + v] * m[ch + a]; }
    for (int i = 0; i < NS; ++i) h[2 * ch + i] = (float)x[2 * N + i] * m[2 * ch + i];
    CTX_HIP(c, ctx_upload(c, c->v_u.p, h.data(), h.size()));
    rc = run_pass(c, PASS_JTJP, p, c->v_u.p, c->v_acc.p); if (rc) return rc;
    CTX_HIP(c, sync_stream(c));
    return vo.vector_to_visit(c, c->v_acc.p, y);
}

int i3d_debug_work_list(i3d_context* c, int32_t* visit_index, int64_t capacity, int64_t* count) {
    CTX_ENTER(c, true, I3D_ERR_INVALID_ARGUMENT);
    if (!visit_index && !count) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_debug_work_list: null pointer");
    if (!c->assembled) return ctx_fail(c, I3D_ERR_STATE, "debug: call i3d_debug_assemble first");
    const int A = c->A;
    if (count) *count = A;
    if (!visit_index) return I3D_OK;
    if (capacity < A) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_debug_work_list: capacity is smaller than the work list");
    VisitOrder vo; if (int rc = vo.fetch(c, true)) return rc;
    CTX_HIP(c, ctx_sync(c));
    for (int a = 0; a < A; ++a) visit_index[a] = vo.of_entry(a);      // the maps vector_to_visit reads
    return I3D_OK;
}

}  // extern "C"
