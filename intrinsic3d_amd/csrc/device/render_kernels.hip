// Ray casting of the resident grid into one camera (i3d_render_view; the definition is DESIGN.md section 13).
//   k_render_bricks<0>  brick bounds of the voxels with weight != 0 (wave min / max, one atomic per wave and axis)
//   k_render_bricks<1>  the dense brick bitmap over those bounds (one atomicOr per run of voxels in the same brick: the grid is brick-sorted)
//   k_render<G>         one lane per pixel, one wave per 8x8 pixel tile (neighbouring rays walk the same bricks), four tiles per workgroup; G = RenderGrid (the
//                       context's grid) or FusionRenderGrid (the fusion table as it stands, DESIGN.md section 15: depth, normal and stats only)
//   k_render<G, true>   the colour view of either: depth, the stored colour interpolated in the hit's cell, the stats
//   k_fusion_bricks_*   the brick bitmap of a fusion table, one lane per slot
// The march runs in fp64 (ray set-up, positions, field values): voxel keys near +-1e5 keep their sub-voxel positions.  Compiled with -ffp-contract=off: the
// numpy statement of the definition (tests/render_twin.py) evaluates the same fp64 expressions in the same order.  The ray, its march and the attributes at a hit
// are ray_march_device.hpp, shared with the caller's own rays (cast_rays_kernels.hip).
#include "render_kernels.hpp"
#include "ray_march_device.hpp"
#include <climits>
#include <type_traits>

namespace i3d {
namespace {

constexpr int TILE = 8;                      // pixels per wave tile edge
constexpr int BLOCK_PX = 2 * TILE;           // a workgroup of 4 waves covers 16 x 16 pixels

template <int FILL>
__global__ void __launch_bounds__(256) k_render_bricks(int N, const int* __restrict__ cx, const int* __restrict__ cy, const int* __restrict__ cz,
                                                       const float* __restrict__ weight, int* __restrict__ bounds, unsigned* __restrict__ bits,
                                                       int lx, int ly, int lz, int dx, int dy) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const bool on = s < N && weight[s] != 0.0f;
    const int bx = on ? brick_of(cx[s]) : 0, by = on ? brick_of(cy[s]) : 0, bz = on ? brick_of(cz[s]) : 0;
    if (!FILL) {
        int mn[3] = {on ? bx : INT_MAX, on ? by : INT_MAX, on ? bz : INT_MAX}, mx[3] = {on ? bx : INT_MIN, on ? by : INT_MIN, on ? bz : INT_MIN};
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int a = 0; a < 3; ++a) { mn[a] = min(mn[a], __shfl_xor(mn[a], o)); mx[a] = max(mx[a], __shfl_xor(mx[a], o)); }
        if ((threadIdx.x & 63) == 0 && mn[0] != INT_MAX)
#pragma unroll
            for (int a = 0; a < 3; ++a) { atomicMin(&bounds[a], mn[a]); atomicMax(&bounds[3 + a], mx[a]); }
    } else {
        const long long idx = on ? ((long long)(bz - lz) * dy + (by - ly)) * dx + (bx - lx) : -1;
        const long long prev = __shfl_up(idx, 1);
        if (on && ((threadIdx.x & 63) == 0 || prev != idx)) atomicOr(&bits[idx >> 5], 1u << (unsigned)(idx & 31));
    }
}

// the fusion table's slots with weight != 0: bounds (wave min / max, then the four waves in LDS, at most one atomic per workgroup and axis) and the bitmap fill (the lanes of a
// wave that set the same word are OR-ed together first: slots are in hash order, so a wave's bricks are scattered and a run rule would not combine anything)
__device__ inline bool fusion_slot_brick(const FusionTable& t, unsigned long long s, int (&b)[3]) {
    if (s > t.mask) return false;
    const unsigned long long k = t.keys[s];
    if (k == FUSION_EMPTY || t.weight[s] == 0.0f) return false;
    int x, y, z; fusion_hash::unpack_key(k, x, y, z);
    b[0] = brick_of(x); b[1] = brick_of(y); b[2] = brick_of(z);
    return true;
}

__global__ void __launch_bounds__(256) k_fusion_bricks_bounds(FusionTable t, int* __restrict__ bounds) {
    __shared__ int red[4][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int b[3] = {0, 0, 0};
    const bool on = fusion_slot_brick(t, (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x, b);
    int mn[3] = {on ? b[0] : INT_MAX, on ? b[1] : INT_MAX, on ? b[2] : INT_MAX}, mx[3] = {on ? b[0] : INT_MIN, on ? b[1] : INT_MIN, on ? b[2] : INT_MIN};
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = min(mn[a], __shfl_xor(mn[a], o)); mx[a] = max(mx[a], __shfl_xor(mx[a], o)); }
    if (lane == 0)
#pragma unroll
        for (int a = 0; a < 3; ++a) { red[wave][a] = mn[a]; red[wave][3 + a] = mx[a]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        int r = red[0][a];
        for (int w = 1; w < 4; ++w) r = a < 3 ? min(r, red[w][a]) : max(r, red[w][a]);
        // only a workgroup that widens the bound so far issues its atomic: 2^26 slots are 2^18 workgroups on six words (the read may be stale, which costs
        // an atomic, never a bound)
        const int cur = bounds[a];
        if (a < 3 ? r < cur : r > cur) { if (a < 3) atomicMin(&bounds[a], r); else atomicMax(&bounds[a], r); }
    }
}

__global__ void __launch_bounds__(256) k_fusion_bricks_fill(FusionTable t, unsigned* __restrict__ bits, int lx, int ly, int lz, int dx, int dy) {
    const int lane = threadIdx.x & 63;
    int b[3] = {0, 0, 0};
    const bool on = fusion_slot_brick(t, (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x, b);
    const long long idx = on ? ((long long)(b[2] - lz) * dy + (b[1] - ly)) * dx + (b[0] - lx) : 0;
    const long long word = on ? idx >> 5 : -1;
    const unsigned bit = on ? 1u << (unsigned)(idx & 31) : 0u;
    unsigned long long pending = __ballot(on);
    while (pending) {                                      // one round per distinct word of the wave
        const int leader = __ffsll((unsigned long long)pending) - 1;
        const long long w = __shfl(word, leader);
        const bool mine = on && word == w;
        unsigned m = mine ? bit : 0u;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor(m, o);
        if (lane == leader) atomicOr(&bits[w], m);
        pending &= ~__ballot(mine);
    }
}

// COLOR: the colour view: depth, the stored colour at the hit and the stats; the normal, albedo, SH and residual code is not in that instantiation
template <class G, bool COLOR = false>
__global__ void __launch_bounds__(256) k_render(G g, RenderCam cam, std::conditional_t<COLOR, RenderColorPlanes, RenderPlanes> out, RenderStatsDev* __restrict__ stats) {
    constexpr bool ATTRIBUTES = std::is_same<G, RenderGrid>::value;     // albedo / SH exist in the context's grid only
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x * BLOCK_PX + (wave & 1) * TILE + (lane & 7), v = blockIdx.y * BLOCK_PX + (wave >> 1) * TILE + (lane >> 3);
    const bool in = u < cam.k.w && v < cam.k.h;
    int samples = 0; bool hit = false; double rsq = 0.0;
    if (in) {
        double x, y; undistort(cam.k, u, v, x, y);                          // the ray through the integer pixel coordinate
        Ray r;
#pragma unroll
        for (int a = 0; a < 3; ++a) { r.eye[a] = cam.eye[a]; r.dir[a] = (cam.R[a] * x + cam.R[3 + a] * y) + cam.R[6 + a]; }
        r.inv_len = 1.0 / sqrt((r.dir[0] * r.dir[0] + r.dir[1] * r.dir[1]) + r.dir[2] * r.dir[2]);
        CellCache cc; cc.b[0] = INT_MIN; cc.b[1] = INT_MIN; cc.b[2] = INT_MIN; cc.valid = false;
        double t_hit = 0.0;
        hit = march(g, cam.tmin, cam.tmax, r, cc, t_hit, samples);
        if constexpr (COLOR) {
            float rgb[3] = {0.0f, 0.0f, 0.0f};
            if (hit && out.color) hit_color(g, cc, rgb);
            const size_t px = (size_t)v * cam.k.w + u;
            if (out.depth) out.depth[px] = hit ? (float)t_hit : 0.0f;
            if (out.color) { out.color[3 * px] = rgb[0]; out.color[3 * px + 1] = rgb[1]; out.color[3 * px + 2] = rgb[2]; }
        } else {
            HitAttr at{{0.0f, 0.0f, 0.0f}, 0.0f, 0.0f, 0.0f}; float o_res = 0.0f;
            if (hit) {
                hit_attributes(g, cc, out.albedo || out.need_sh, out.need_sh != 0, at);
                if (ATTRIBUTES && out.residual) { o_res = at.intensity - out.lum[(size_t)v * cam.k.w + u]; rsq = (double)o_res * (double)o_res; }
            }
            const size_t px = (size_t)v * cam.k.w + u;
            if (out.depth) out.depth[px] = hit ? (float)t_hit : 0.0f;
            if (out.normal) { out.normal[3 * px] = at.n[0]; out.normal[3 * px + 1] = at.n[1]; out.normal[3 * px + 2] = at.n[2]; }
            if (out.albedo) out.albedo[px] = at.albedo;
            if (out.shading) out.shading[px] = at.shading;
            if (out.intensity) out.intensity[px] = at.intensity;
            if (out.residual) out.residual[px] = o_res;
        }
    }
    unsigned long long nh = hit ? 1ull : 0ull, ns = (unsigned long long)samples;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { nh += __shfl_xor(nh, o); ns += __shfl_xor(ns, o); rsq += __shfl_xor(rsq, o); }
    if (lane == 0 && ns > 0) {
        atomicAdd(&stats->hits, nh); atomicAdd(&stats->samples, ns);
        if (rsq != 0.0) atomicAdd(&stats->residual_sq, rsq);
    }
}

}  // namespace

void launch_render_brick_bounds(hipStream_t st, int N, const int* cx, const int* cy, const int* cz, const float* weight, int* bounds) {
    if (N > 0) k_render_bricks<0><<<(N + 255) / 256, 256, 0, st>>>(N, cx, cy, cz, weight, bounds, nullptr, 0, 0, 0, 0, 0);
}
void launch_render_brick_fill(hipStream_t st, int N, const int* cx, const int* cy, const int* cz, const float* weight, unsigned* bits, const int lo[3], const int dim[3]) {
    if (N > 0) k_render_bricks<1><<<(N + 255) / 256, 256, 0, st>>>(N, cx, cy, cz, weight, nullptr, bits, lo[0], lo[1], lo[2], dim[0], dim[1]);
}
void launch_render(hipStream_t st, const RenderGrid& g, const RenderCam& cam, const RenderPlanes& out, RenderStatsDev* stats) {
    const dim3 grid((cam.k.w + BLOCK_PX - 1) / BLOCK_PX, (cam.k.h + BLOCK_PX - 1) / BLOCK_PX);
    k_render<RenderGrid><<<grid, 256, 0, st>>>(g, cam, out, stats);
}
void launch_render_color(hipStream_t st, const RenderGrid& g, const RenderCam& cam, const RenderColorPlanes& out, RenderStatsDev* stats) {
    const dim3 grid((cam.k.w + BLOCK_PX - 1) / BLOCK_PX, (cam.k.h + BLOCK_PX - 1) / BLOCK_PX);
    k_render<RenderGrid, true><<<grid, 256, 0, st>>>(g, cam, out, stats);
}
void launch_fusion_brick_bounds(hipStream_t st, const FusionTable& t, int* bounds) {
    k_fusion_bricks_bounds<<<(unsigned)((t.mask + 1 + 255) / 256), 256, 0, st>>>(t, bounds);
}
void launch_fusion_brick_fill(hipStream_t st, const FusionTable& t, unsigned* bits, const int lo[3], const int dim[3]) {
    k_fusion_bricks_fill<<<(unsigned)((t.mask + 1 + 255) / 256), 256, 0, st>>>(t, bits, lo[0], lo[1], lo[2], dim[0], dim[1]);
}
void launch_render(hipStream_t st, const FusionRenderGrid& g, const RenderCam& cam, const RenderPlanes& out, RenderStatsDev* stats) {
    const dim3 grid((cam.k.w + BLOCK_PX - 1) / BLOCK_PX, (cam.k.h + BLOCK_PX - 1) / BLOCK_PX);
    k_render<FusionRenderGrid><<<grid, 256, 0, st>>>(g, cam, out, stats);
}
void launch_render_color(hipStream_t st, const FusionRenderGrid& g, const RenderCam& cam, const RenderColorPlanes& out, RenderStatsDev* stats) {
    const dim3 grid((cam.k.w + BLOCK_PX - 1) / BLOCK_PX, (cam.k.h + BLOCK_PX - 1) / BLOCK_PX);
    k_render<FusionRenderGrid, true><<<grid, 256, 0, st>>>(g, cam, out, stats);
}

}  // namespace i3d
