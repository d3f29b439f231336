// i3d_query_points: the stored field at arbitrary world points and their projection onto its zero level set (query_kernels.hip; the definition is DESIGN.md
// section 17).  query_run is the driver for every model (model.hpp: the context here, the fusion volume in fusion.cpp): validation, the model's grown-only
// scratch, two launches, the requested arrays copied back, one stream synchronisation.  Reads the grid; writes only its scratch, nothing any other entry point reads.
#include "context.hpp"

using namespace i3d;

namespace i3d {

int query_run(const Model& m, const i3d_query_desc* d, int64_t n, const double* points, double* sdf, float* normal, float* albedo, double* foot, double* distance,
              uint8_t* status, i3d_query_stats* stats) {
    constexpr int64_t QUERY_MAX_POINTS = 1ll << 27;
    const std::string& fn = m.fn;
    hipStream_t st = m.stream; DevBuf<unsigned char>& scratch = m.buf.query_scratch;
    if (!d) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null descriptor");
    if (n < 0 || n > QUERY_MAX_POINTS) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": n must be 0.." + std::to_string(QUERY_MAX_POINTS) + " (2^27)");
    if (n > 0 && !points) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null points");
    if (d->max_steps < 0 || d->max_steps > QUERY_MAX_STEPS) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": max_steps must be 0.." + std::to_string(QUERY_MAX_STEPS));
    if (!std::isfinite(d->tolerance_voxels) || !(d->tolerance_voxels > 0.0)) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": tolerance_voxels must be finite and > 0");
    if (!d->project && (foot || distance)) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": foot / distance need project = 1");
    if (int rc = m.ready()) return rc;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (n == 0) return I3D_OK;

    // the scratch: points | the requested outputs | one row per workgroup | the total; every piece 256-byte aligned
    const size_t N = (size_t)n, rows = (size_t)query_rows(n);
    size_t total = 0;
    auto take = [&total](bool wanted, size_t bytes) { const size_t at = total; if (wanted) total += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_pts = take(true, 24 * N), o_sdf = take(sdf, 8 * N), o_foot = take(foot, 24 * N), o_dist = take(distance, 8 * N), o_nrm = take(normal, 12 * N),
                 o_alb = take(albedo, 4 * N), o_st = take(status, N), o_rows = take(true, rows * sizeof(QueryRow)), o_tot = take(true, sizeof(QueryRow));
    MODEL_HIP(m, scratch.alloc(total));
    unsigned char* base = scratch.p;
    const QueryOut out{sdf ? (double*)(base + o_sdf) : nullptr, normal ? (float*)(base + o_nrm) : nullptr, albedo ? (float*)(base + o_alb) : nullptr,
                       foot ? (double*)(base + o_foot) : nullptr, distance ? (double*)(base + o_dist) : nullptr, status ? base + o_st : nullptr};
    const QueryParams prm{(long long)n, d->project ? 1 : 0, d->max_steps, d->tolerance_voxels * m.voxel_size};
    MODEL_HIP(m, hipMemcpyAsync(base + o_pts, points, 24 * N, hipMemcpyHostToDevice, st));
    m.query(prm, (const double*)(base + o_pts), out, (QueryRow*)(base + o_rows), (QueryRow*)(base + o_tot));
    MODEL_HIP(m, hipGetLastError());
    auto back = [&](void* dst, const void* src, size_t bytes) -> hipError_t { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
    MODEL_HIP(m, back(sdf, out.sdf, 8 * N)); MODEL_HIP(m, back(normal, out.normal, 12 * N)); MODEL_HIP(m, back(albedo, out.albedo, 4 * N));
    MODEL_HIP(m, back(foot, out.foot, 24 * N)); MODEL_HIP(m, back(distance, out.distance, 8 * N)); MODEL_HIP(m, back(status, out.status, N));
    QueryRow t{};
    MODEL_HIP(m, hipMemcpyAsync(&t, base + o_tot, sizeof(t), hipMemcpyDeviceToHost, st));
    MODEL_HIP(m, hipStreamSynchronize(st));
    if (stats) {
        stats->valid = t.valid; stats->projected = t.projected; stats->steps = t.steps;
        stats->sum_abs_sdf = t.sum_abs_sdf; stats->sum_sq_sdf = t.sum_sq_sdf; stats->max_abs_sdf = t.max_abs_sdf;
        stats->sum_abs_distance = t.sum_abs_distance; stats->sum_sq_distance = t.sum_sq_distance; stats->max_abs_distance = t.max_abs_distance;
    }
    return I3D_OK;
}

}  // namespace i3d

extern "C" void i3d_query_desc_default(i3d_query_desc* d) {
    if (!d) return;
    std::memset(d, 0, sizeof(*d));
    d->use_refined_sdf = 1; d->project = 1; d->max_steps = 16; d->tolerance_voxels = 1e-6;
}

extern "C" int i3d_query_points(i3d_context* c, const i3d_query_desc* d, int64_t n, const double* points, double* sdf, float* normal, float* albedo, double* foot,
                                double* distance, uint8_t* status, i3d_query_stats* stats) {
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_query_points: null context");
    return query_run(ContextModel(c, "i3d_query_points", d && d->use_refined_sdf != 0), d, n, points, sdf, normal, albedo, foot, distance, status, stats);
}
