// i3d_cast_rays / i3d_cast_rays_color: the caller's own rays on the stored field (cast_rays_kernels.hip; the definition is DESIGN.md section 34, the colour 35).  cast_rays_run is the driver for
// every model (model.hpp: the context here, the fusion volume in fusion.cpp): validation, the cached brick bitmap, the model's grown-only scratch, with
// order = 1 the key kernel and the sort, one march launch, the requested arrays copied back, one stream synchronisation (plus the one of a bitmap rebuild).
// Reads the grid and the SH; writes only the model's buffers (bitmap, scratch), nothing any other entry point reads.
#include "context.hpp"
#include <algorithm>

using namespace i3d;

namespace i3d {

int cast_rays_run(const Model& m, bool have_sh, int32_t order, int64_t n, const double* origins, const double* directions, const double* t_min, const double* t_max, double* t,
                  double* position, float* normal, float* albedo, float* shading, float* intensity, uint8_t* status, i3d_render_stats* stats, bool colour_call,
                  float* color) {
    if (!colour_call) color = nullptr;
    constexpr int64_t CAST_MAX_RAYS = 1ll << 27;
    const std::string& fn = m.fn;
    hipStream_t st = m.stream; DevBuf<unsigned char>& scratch = m.buf.cast_scratch;
    if (n < 0 || n > CAST_MAX_RAYS) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": n must be 0.." + std::to_string(CAST_MAX_RAYS) + " (2^27)");
    if (n > 0 && (!origins || !directions)) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": null origins / directions");
    if (order != 0 && order != 1) return m.fail(I3D_ERR_INVALID_ARGUMENT, fn + ": order must be 0 (as given) or 1 (the coherent order)");
    if (int rc = m.check_field()) return rc;
    if ((shading || intensity) && !have_sh) return m.fail(I3D_ERR_STATE, fn + ": shading and intensity need the per-voxel SH (i3d_set_voxel_sh / i3d_estimate_sh)");
    if (n == 0) { if (stats) std::memset(stats, 0, sizeof(*stats)); return I3D_OK; }
    if (int rc = m.make_current()) return rc;
    if (int rc = ensure_bricks(m)) return rc;

    // the scratch: origins | directions | ranges | the requested outputs (of a colour call: t, colour, status) | with order = 1 keys, indices (each in and out) and the sort's storage | the stats;
    // every piece 256-byte aligned
    const size_t N = (size_t)n;
    const ModelBuffers::Bricks& k = m.buf.bricks;
    const int coord_bits = cast_coord_bits(k.dim), key_bits = cast_key_bits(coord_bits);
    const size_t sort_bytes = order ? std::max(cast_sort_temp_bytes(n, key_bits), (size_t)256) : 0;
    size_t total = 0;
    auto take = [&total](bool wanted, size_t bytes) { const size_t at = total; if (wanted) total += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_org = take(true, 24 * N), o_dir = take(true, 24 * N), o_tmin = take(t_min, 8 * N), o_tmax = take(t_max, 8 * N), o_t = take(t, 8 * N),
                 o_pos = take(position, 24 * N), o_nrm = take(normal, 12 * N), o_alb = take(albedo, 4 * N), o_sh = take(shading, 4 * N), o_int = take(intensity, 4 * N),
                 o_col = take(color, 12 * N), o_st = take(status, N), o_key0 = take(order, 8 * N), o_key1 = take(order, 8 * N), o_idx0 = take(order, 4 * N), o_idx1 = take(order, 4 * N),
                 o_sort = take(order, sort_bytes), o_stats = take(true, sizeof(RenderStatsDev));
    MODEL_HIP(m, scratch.alloc(total));
    unsigned char* base = scratch.p;
    CastRaysColor p{};
    p.n = (long long)n;
    p.origins = (const double*)(base + o_org); p.directions = (const double*)(base + o_dir);
    p.t_min = t_min ? (const double*)(base + o_tmin) : nullptr; p.t_max = t_max ? (const double*)(base + o_tmax) : nullptr;
    p.perm = nullptr;
    p.t = t ? (double*)(base + o_t) : nullptr; p.position = position ? (double*)(base + o_pos) : nullptr; p.normal = normal ? (float*)(base + o_nrm) : nullptr;
    p.albedo = albedo ? (float*)(base + o_alb) : nullptr; p.shading = shading ? (float*)(base + o_sh) : nullptr; p.intensity = intensity ? (float*)(base + o_int) : nullptr;
    p.status = status ? base + o_st : nullptr;
    p.color = color ? (float*)(base + o_col) : nullptr;
    p.need_sh = shading || intensity ? 1 : 0;
    RenderStatsDev* dstats = (RenderStatsDev*)(base + o_stats);

    MODEL_HIP(m, hipMemcpyAsync(base + o_org, origins, 24 * N, hipMemcpyHostToDevice, st));
    MODEL_HIP(m, hipMemcpyAsync(base + o_dir, directions, 24 * N, hipMemcpyHostToDevice, st));
    if (t_min) MODEL_HIP(m, hipMemcpyAsync(base + o_tmin, t_min, 8 * N, hipMemcpyHostToDevice, st));
    if (t_max) MODEL_HIP(m, hipMemcpyAsync(base + o_tmax, t_max, 8 * N, hipMemcpyHostToDevice, st));
    MODEL_HIP(m, hipMemsetAsync(dstats, 0, sizeof(RenderStatsDev), st));
    if (order) {
        CastBox box{m.voxel_size, {k.lo[0], k.lo[1], k.lo[2]}, {k.dim[0], k.dim[1], k.dim[2]}};
        launch_cast_ray_keys(st, box, p, coord_bits, (unsigned long long*)(base + o_key0), (unsigned*)(base + o_idx0));
        MODEL_HIP(m, hipGetLastError());
        MODEL_HIP(m, launch_cast_sort(st, base + o_sort, sort_bytes, (const unsigned long long*)(base + o_key0), (unsigned long long*)(base + o_key1),
                                      (const unsigned*)(base + o_idx0), (unsigned*)(base + o_idx1), (long long)n, key_bits));
        p.perm = (const unsigned*)(base + o_idx1);
    }
    if (colour_call) m.cast_rays_color(p, dstats);
    else m.cast_rays(p, dstats);
    MODEL_HIP(m, hipGetLastError());
    auto back = [&](void* dst, const void* src, size_t bytes) -> hipError_t { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess; };
    MODEL_HIP(m, back(t, p.t, 8 * N)); MODEL_HIP(m, back(position, p.position, 24 * N)); MODEL_HIP(m, back(normal, p.normal, 12 * N));
    MODEL_HIP(m, back(albedo, p.albedo, 4 * N)); MODEL_HIP(m, back(shading, p.shading, 4 * N)); MODEL_HIP(m, back(intensity, p.intensity, 4 * N));
    MODEL_HIP(m, back(color, p.color, 12 * N)); MODEL_HIP(m, back(status, p.status, N));
    RenderStatsDev s{};
    MODEL_HIP(m, hipMemcpyAsync(&s, dstats, sizeof(s), hipMemcpyDeviceToHost, st));
    MODEL_HIP(m, hipStreamSynchronize(st));
    if (stats) { stats->hits = (int64_t)s.hits; stats->samples = (int64_t)s.samples; stats->residual_sq_sum = 0.0; }
    return I3D_OK;
}

}  // namespace i3d

extern "C" int i3d_cast_rays(i3d_context* c, int32_t use_refined_sdf, int32_t order, int64_t n, const double* origins, const double* directions, const double* t_min,
                             const double* t_max, double* t, double* position, float* normal, float* albedo, float* shading, float* intensity, uint8_t* status,
                             i3d_render_stats* stats) {
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_cast_rays: null context");
    return cast_rays_run(ContextModel(c, "i3d_cast_rays", use_refined_sdf != 0), c->have_sh, order, n, origins, directions, t_min, t_max, t, position, normal, albedo, shading,
                         intensity, status, stats);
}

// the colour call: t, status and the stored colour at the hit; no SH is read
extern "C" int i3d_cast_rays_color(i3d_context* c, int32_t use_refined_sdf, int32_t order, int64_t n, const double* origins, const double* directions, const double* t_min,
                                   const double* t_max, double* t, float* color, uint8_t* status, i3d_render_stats* stats) {
    if (!c) return ctx_fail(c, I3D_ERR_INVALID_ARGUMENT, "i3d_cast_rays_color: null context");
    return cast_rays_run(ContextModel(c, "i3d_cast_rays_color", use_refined_sdf != 0), false, order, n, origins, directions, t_min, t_max, t, nullptr, nullptr, nullptr, nullptr,
                         nullptr, status, stats, true, color);
}
