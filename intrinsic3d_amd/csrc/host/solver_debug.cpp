// Parity probes of the assembled normal equations (i3d_debug_normal_equations / _jtj_apply / _work_list): the passes of pcg.cpp on the rows of the last
// i3d_debug_assemble, handed back in visit order.
#include "solver_internal.hpp"

namespace i3d {

static int list_maps(i3d_context* c, std::vector<int>& rank, std::vector<int>& alist) {
    rank.resize(c->N); alist.resize(c->A > 0 ? c->A : 1);
    CTX_HIP(c, hipMemcpy(rank.data(), c->rank.p, sizeof(int) * (size_t)c->N, hipMemcpyDeviceToHost));
    if (c->A > 0) CTX_HIP(c, hipMemcpy(alist.data(), c->alist.p, sizeof(int) * (size_t)c->A, hipMemcpyDeviceToHost));
    return I3D_OK;
}
static int to_visit_order(i3d_context* c, const float* dev_vec, double* out) {
    const int N = c->N, A = c->A, K = c->K, NS = 6 * K + 9, ch = c->shard.chunk, NP = 2 * ch + NS;      // single-rank layout [sdf ch | alb ch | camera]
    std::vector<float> h(NP); std::vector<int> rank, alist;
    CTX_HIP(c, hipMemcpy(h.data(), dev_vec, sizeof(float) * (size_t)NP, hipMemcpyDeviceToHost));
    int rc = list_maps(c, rank, alist); if (rc) return rc;
    for (int i = 0; i < 2 * N + NS; ++i) out[i] = 0.0;
    for (int a = 0; a < A; ++a) { const int v = rank[alist[a]]; out[v] = h[a]; out[N + v] = h[ch + a]; }
    for (int i = 0; i < NS; ++i) out[2 * N + i] = h[2 * ch + i];
    return I3D_OK;
}

int normal_eq_debug(i3d_context* c, double* gradient, double* jtj_diag, double* cost) {
    if (!c->assembled) return ctx_fail(c, I3D_ERR_STATE, "debug: call i3d_debug_assemble first");
    CTX_HIP(c, hipSetDevice(c->device));
    OptParams p = c->last_params;
    launch_freemask(c->stream, c->row_view(), p, c->v_mask.p);
    int rc;
    if (jtj_diag) { rc = run_pass(c, PASS_COLNORM, p, nullptr, c->v_c.p); if (rc) return rc; CTX_HIP(c, sync_stream(c)); rc = to_visit_order(c, c->v_c.p, jtj_diag); if (rc) return rc; }
    if (gradient) { rc = run_pass(c, PASS_GRAD, p, nullptr, c->v_acc.p); if (rc) return rc; CTX_HIP(c, sync_stream(c)); rc = to_visit_order(c, c->v_acc.p, gradient); if (rc) return rc; }
    if (cost) {
        rc = eval_cost_launch(c, p, false, c->d_frames.p); if (rc) return rc;
        rc = read_doubles(c, c->d_scal.p + 16, 1, cost); if (rc) return rc;
        if (c->sharded() && c->comm->health(c->stream)) return ctx_fail(c, I3D_ERR_COMM, "cost evaluation: a peer-to-peer exchange timed out (a rank stopped taking part)");
    }
    return I3D_OK;
}

int jtj_apply_debug(i3d_context* c, const double* x, double* y) {
    if (!c->assembled) return ctx_fail(c, I3D_ERR_STATE, "debug: call i3d_debug_assemble first");
    CTX_HIP(c, hipSetDevice(c->device));
    const int N = c->N, A = c->A, K = c->K, NS = 6 * K + 9, ch = c->shard.chunk, NP = 2 * ch + NS;
    OptParams p = c->last_params;
    std::vector<int> rank, alist; std::vector<float> h(NP, 0.0f), m(NP);
    int rc = list_maps(c, rank, alist); if (rc) return rc;
    launch_freemask(c->stream, c->row_view(), p, c->v_mask.p);
    CTX_HIP(c, sync_stream(c));
    CTX_HIP(c, hipMemcpy(m.data(), c->v_mask.p, sizeof(float) * (size_t)NP, hipMemcpyDeviceToHost));
    for (int a = 0; a < A; ++a) { const int v = rank[alist[a]]; h[a] = (float)x[v] * m[a]; h[ch + a] = (float)x[N + v] * m[ch + a]; }
    for (int i = 0; i < NS; ++i) h[2 * ch + i] = (float)x[2 * N + i] * m[2 * ch + i];
    CTX_HIP(c, hipMemcpy(c->v_u.p, h.data(), sizeof(float) * (size_t)NP, hipMemcpyHostToDevice));
    rc = run_pass(c, PASS_JTJP, p, c->v_u.p, c->v_acc.p); if (rc) return rc;
    CTX_HIP(c, sync_stream(c));
    return to_visit_order(c, c->v_acc.p, y);
}

int work_list_debug(i3d_context* c, int32_t* visit_index, int64_t capacity, int64_t* count) {
    if (!c->assembled) return ctx_fail(c, I3D_ERR_STATE, "debug: call i3d_debug_assemble first");
    CTX_HIP(c, hipSetDevice(c->device));
    const int A = c->A;
    if (count) *count = A;
    if (!visit_index) return I3D_OK;
    if (capacity < A) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_debug_work_list: capacity is smaller than the work list");
    std::vector<int> rank, alist;
    int rc = list_maps(c, rank, alist); if (rc) return rc;
    for (int a = 0; a < A; ++a) visit_index[a] = rank[alist[a]];      // the maps to_visit_order reads
    return I3D_OK;
}

}  // namespace i3d
