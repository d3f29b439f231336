// The caller's own rays on the stored field (i3d_cast_rays / i3d_fusion_cast_rays; the definition is DESIGN.md section 34).
//   k_cast_rays<G>    one lane per ray: the ray read and checked, the march and the hit attributes of ray_march_device.hpp (the ones k_render runs), every
//                     requested output written at the ray's own index; G = RenderGrid or FusionRenderGrid (t, position, normal, status only)
//   k_cast_rays<G, true>  the colour call of either: t, status, the stored colour interpolated in the hit's cell, the stats
//   k_cast_ray_keys   the coherent order: one sort key per ray from its direction's sign octant and the brick at its entry into the bitmap's box
// A wave costs its longest ray and rays that walk different bricks scatter their hash probes, so with order = 1 the keys are sorted (rocprim) and lane j marches
// ray perm[j]: which lane marches a ray changes nothing it computes.  fp64 and -ffp-contract=off as render_kernels.hip: the numpy statement is
// tests/cast_rays_twin.py.
#include "cast_rays_kernels.hpp"
#include "ray_march_device.hpp"
#include <climits>
#include <cstring>
#include <rocprim/rocprim.hpp>

namespace i3d {
namespace {

// ray i and its range [a, b); false: the ray is invalid and is not marched
__device__ inline bool load_ray(const CastRays& p, double vs, long long i, Ray& r, double& a, double& b) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.eye[k] = p.origins[3 * i + k]; r.dir[k] = p.directions[3 * i + k];
        ok = ok && isfinite(r.eye[k]) && isfinite(r.dir[k]) && fabs(r.eye[k] / vs) < QUERY_MAX_COORD;
    }
    const double l2 = (r.dir[0] * r.dir[0] + r.dir[1] * r.dir[1]) + r.dir[2] * r.dir[2];
    const double lo = p.t_min ? p.t_min[i] : 0.0, hi = p.t_max ? p.t_max[i] : 0.0;
    ok = ok && l2 > 0.0 && isfinite(l2) && lo == lo && hi == hi && !(lo > 0.0 && isinf(lo));
    a = lo > 0.0 ? lo : 0.0;
    b = hi > 0.0 ? hi : (double)INFINITY;
    r.inv_len = 1.0 / sqrt(l2);
    return ok;
}

// COLOR: the colour call: t, status, the stored colour at the hit and the stats; the position, normal, albedo and SH code is not in that instantiation
template <class G, bool COLOR = false>
__global__ void __launch_bounds__(CAST_BLOCK) k_cast_rays(G g, std::conditional_t<COLOR, CastRaysColor, CastRays> p, RenderStatsDev* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const long long j = (long long)blockIdx.x * CAST_BLOCK + threadIdx.x;
    int samples = 0; bool hit = false;
    if (j < p.n) {
        const long long i = p.perm ? (long long)p.perm[j] : j;
        Ray r; double a, b;
        const bool valid = load_ray(p, g.vs, i, r, a, b);
        double t_hit = 0.0;
        if constexpr (COLOR) {
            float rgb[3] = {0.0f, 0.0f, 0.0f};
            if (valid) {
                CellCache cc; cell_cache_reset(cc);
                hit = march(g, a, b, r, cc, t_hit, samples);
                if (hit && p.color) hit_color(g, cc, rgb);
            }
            if (p.t) p.t[i] = hit ? t_hit : 0.0;
            if (p.color) { p.color[3 * i] = rgb[0]; p.color[3 * i + 1] = rgb[1]; p.color[3 * i + 2] = rgb[2]; }
        } else {
            HitAttr at{{0.0f, 0.0f, 0.0f}, 0.0f, 0.0f, 0.0f};
            if (valid) {
                CellCache cc; cell_cache_reset(cc);
                hit = march(g, a, b, r, cc, t_hit, samples);
                if (hit) hit_attributes(g, cc, p.albedo || p.need_sh, p.need_sh != 0, at);
            }
            if (p.t) p.t[i] = hit ? t_hit : 0.0;
            if (p.position)
#pragma unroll
                for (int k = 0; k < 3; ++k) p.position[3 * i + k] = hit ? r.eye[k] + t_hit * r.dir[k] : 0.0;
            if (p.normal) { p.normal[3 * i] = at.n[0]; p.normal[3 * i + 1] = at.n[1]; p.normal[3 * i + 2] = at.n[2]; }
            if (p.albedo) p.albedo[i] = at.albedo;
            if (p.shading) p.shading[i] = at.shading;
            if (p.intensity) p.intensity[i] = at.intensity;
        }
        if (p.status)
            p.status[i] = (unsigned char)(valid ? CAST_VALID | (hit ? CAST_HIT : 0) | (!hit && samples >= RENDER_MAX_SAMPLES ? CAST_BUDGET : 0) : 0);
    }
    unsigned long long nh = hit ? 1ull : 0ull, ns = (unsigned long long)samples;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nh += __shfl_xor(nh, o); ns += __shfl_xor(ns, o); }
    if (lane == 0 && ns > 0) { atomicAdd(&stats->hits, nh); atomicAdd(&stats->samples, ns); }
}

// bit i of x -> bit 3 i (x < 2^21)
__device__ inline unsigned long long spread3(unsigned x) {
    unsigned long long v = x & 0x1fffffull;
    v = (v | (v << 32)) & 0x1f00000000ffffull;
    v = (v | (v << 16)) & 0x1f0000ff0000ffull;
    v = (v | (v << 8)) & 0x100f00f00f00f00full;
    v = (v | (v << 4)) & 0x10c30c30c30c30c3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}

__global__ void __launch_bounds__(CAST_BLOCK) k_cast_ray_keys(CastBox g, CastRays p, int coord_bits, unsigned long long* __restrict__ keys, unsigned* __restrict__ index) {
    const long long j = (long long)blockIdx.x * CAST_BLOCK + threadIdx.x;
    if (j >= p.n) return;
    unsigned long long key = 1ull << (3 * coord_bits + 3);              // invalid, or no part of the range inside the box: the largest key
    Ray r; double t0, t1;
    if (load_ray(p, g.vs, j, r, t0, t1)) {
        ray_clip(g, r, t0, t1);
        if (t0 < t1) {
            double q[3]; int b[3]; ray_pos(r, g.vs, t0, q, b);
            unsigned k[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) k[a] = (unsigned)min(max(brick_of(b[a]) - g.lo[a], 0), g.dim[a] - 1);
            const unsigned long long oct = (r.dir[0] < 0.0 ? 1u : 0u) | (r.dir[1] < 0.0 ? 2u : 0u) | (r.dir[2] < 0.0 ? 4u : 0u);
            key = (oct << (3 * coord_bits)) | spread3(k[0]) | (spread3(k[1]) << 1) | (spread3(k[2]) << 2);
        }
    }
    keys[j] = key; index[j] = (unsigned)j;
}

}  // namespace

void launch_cast_rays(hipStream_t st, const RenderGrid& g, const CastRays& p, RenderStatsDev* stats) {
    if (p.n > 0) k_cast_rays<RenderGrid><<<(unsigned)((p.n + CAST_BLOCK - 1) / CAST_BLOCK), CAST_BLOCK, 0, st>>>(g, p, stats);
}
void launch_cast_rays(hipStream_t st, const FusionRenderGrid& g, const CastRays& p, RenderStatsDev* stats) {
    if (p.n > 0) k_cast_rays<FusionRenderGrid><<<(unsigned)((p.n + CAST_BLOCK - 1) / CAST_BLOCK), CAST_BLOCK, 0, st>>>(g, p, stats);
}
void launch_cast_rays_color(hipStream_t st, const RenderGrid& g, const CastRaysColor& p, RenderStatsDev* stats) {
    if (p.n > 0) k_cast_rays<RenderGrid, true><<<(unsigned)((p.n + CAST_BLOCK - 1) / CAST_BLOCK), CAST_BLOCK, 0, st>>>(g, p, stats);
}
void launch_cast_rays_color(hipStream_t st, const FusionRenderGrid& g, const CastRaysColor& p, RenderStatsDev* stats) {
    if (p.n > 0) k_cast_rays<FusionRenderGrid, true><<<(unsigned)((p.n + CAST_BLOCK - 1) / CAST_BLOCK), CAST_BLOCK, 0, st>>>(g, p, stats);
}
void launch_cast_ray_keys(hipStream_t st, const CastBox& box, const CastRays& p, int coord_bits, unsigned long long* keys, unsigned* index) {
    if (p.n > 0) k_cast_ray_keys<<<(unsigned)((p.n + CAST_BLOCK - 1) / CAST_BLOCK), CAST_BLOCK, 0, st>>>(box, p, coord_bits, keys, index);
}
size_t cast_sort_temp_bytes(long long n, int key_bits) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, (const unsigned*)nullptr, (unsigned*)nullptr,
                                    (size_t)n, 0, (unsigned)key_bits, (hipStream_t)0);
    return bytes;
}
hipError_t launch_cast_sort(hipStream_t st, void* temp, size_t temp_bytes, const unsigned long long* keys_in, unsigned long long* keys_out, const unsigned* index_in,
                            unsigned* index_out, long long n, int key_bits) {
    if (n <= 0) return hipSuccess;
    return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, index_in, index_out, (size_t)n, 0, (unsigned)key_bits, st);
}

}  // namespace i3d
