// Ray casting of the resident grid into one camera (i3d_render_view; the definition is DESIGN.md section 13).
//   k_render_bricks<0>  brick bounds of the voxels with weight != 0 (wave min / max, one atomic per wave and axis)
//   k_render_bricks<1>  the dense brick bitmap over those bounds (one atomicOr per run of voxels in the same brick: the grid is brick-sorted)
//   k_render<G>         one lane per pixel, one wave per 8x8 pixel tile (neighbouring rays walk the same bricks), four tiles per workgroup; G = RenderGrid (the
//                       context's grid) or FusionRenderGrid (the fusion table as it stands, DESIGN.md section 15: depth, normal and stats only)
//   k_fusion_bricks_*   the brick bitmap of a fusion table, one lane per slot
// The march runs in fp64 (ray set-up, positions, field values): voxel keys near +-1e5 keep their sub-voxel positions.  Compiled with -ffp-contract=off: the
// numpy statement of the definition (tests/render_twin.py) evaluates the same fp64 expressions in the same order.
#include "render_kernels.hpp"
#include "cell_device.hpp"
#include <climits>
#include <type_traits>

namespace i3d {
namespace {

constexpr int TILE = 8;                      // pixels per wave tile edge
constexpr int BLOCK_PX = 2 * TILE;           // a workgroup of 4 waves covers 16 x 16 pixels

__device__ inline int brick_of(int k) { return k >> RENDER_BRICK_SHIFT; }      // floor(k / 8)

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

// ---- one ray ------------------------------------------------------------------------------------------------------------------------
struct Ray { double eye[3], dir[3], inv_len; };

// the position under the ray at t in voxel units q = (eye + t d) / vs and its cell base = floor(q) (the cell itself: cell_device.hpp)
__device__ inline void ray_pos(const Ray& r, double vs, double t, double (&q)[3], int (&b)[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { q[a] = (r.eye[a] + t * r.dir[a]) / vs; b[a] = (int)floor(q[a]); }
}

template <class G>
__device__ inline bool field_at(const G& g, const Ray& r, CellCache& cc, double t, double& f) {
    double q[3]; int b[3]; ray_pos(r, g.vs, t, q, b);
    if (!cell_at(g, cc, q, b)) return false;
    f = field(cc);
    return true;
}

// the march of DESIGN.md 13.1, steps 3-5; returns the hit and leaves the cell of the attributes in cc
template <class G>
__device__ inline bool march(const G& g, const RenderCam& cam, const Ray& r, CellCache& cc, double& t_hit, int& samples) {
    const double vs = g.vs, dl = vs * r.inv_len;          // one voxel of world length along the ray, in units of t (camera z)
    double t0 = cam.tmin, t1 = cam.tmax;
#pragma unroll
    for (int a = 0; a < 3; ++a) {                          // entry / exit of the bitmap's box [8 lo, 8 (lo + dim)) in voxel units
        const double B0 = (double)(g.lo[a] * 8) * vs, B1 = (double)((g.lo[a] + g.dim[a]) * 8) * vs;
        if (r.dir[a] != 0.0) {
            const double ta = (B0 - r.eye[a]) / r.dir[a], tb = (B1 - r.eye[a]) / r.dir[a];
            t0 = fmax(t0, fmin(ta, tb)); t1 = fmin(t1, fmax(ta, tb));
        } else if (r.eye[a] < B0 || r.eye[a] >= B1) {
            t1 = -1.0;
        }
    }
    bool pv = false; double pt = 0.0, pf = 0.0;
    double t = t0;
    while (t < t1 && samples < RENDER_MAX_SAMPLES) {
        ++samples;
        double q[3]; int b[3]; ray_pos(r, vs, t, q, b);
        const int kx = brick_of(b[0]) - g.lo[0], ky = brick_of(b[1]) - g.lo[1], kz = brick_of(b[2]) - g.lo[2];
        if (kx < 0 || ky < 0 || kz < 0 || kx >= g.dim[0] || ky >= g.dim[1] || kz >= g.dim[2]) { pv = false; t += 1e-4 * dl; continue; }
        const long long bi = ((long long)kz * g.dim[1] + ky) * g.dim[0] + kx;
        if (!((g.bits[bi >> 5] >> (unsigned)(bi & 31)) & 1u)) {          // empty brick: jump to its exit
            double te = t1;
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (r.dir[a] != 0.0) {
                    const int kb = brick_of(b[a]);
                    const double edge = (double)((r.dir[a] > 0.0 ? kb + 1 : kb) * 8) * vs;
                    te = fmin(te, (edge - r.eye[a]) / r.dir[a]);
                }
            pv = false; t = fmax(t, te) + 1e-4 * dl;
            continue;
        }
        if (!cell_at(g, cc, q, b)) { pv = false; t += 0.5 * dl; continue; }
        const double f = field(cc);
        if (f > 0.0) { pv = true; pt = t; pf = f; t += fmin(fmax(f, 0.25 * vs), vs) * r.inv_len; continue; }
        if (pv && pf > 0.0) {                                               // zero crossing from outside: two secant steps on [pt, t]
            double ta = pt, fa = pf, tb = t, fb = f;
            const double tc = ta + (tb - ta) * fa / (fa - fb);
            double fc;
            if (!field_at(g, r, cc, tc, fc)) { t_hit = tc; }
            else {
                if (fc > 0.0) { ta = tc; fa = fc; } else { tb = tc; fb = fc; }
                t_hit = ta + (tb - ta) * fa / (fa - fb);
            }
            double fh;
            if (!field_at(g, r, cc, t_hit, fh)) field_at(g, r, cc, t, fh);  // attributes from the hit sample's cell when t_hit's cell is not valid
            return true;
        }
        pv = true; pt = t; pf = f; t += 0.25 * dl;
    }
    return false;
}

template <class G>
__global__ void __launch_bounds__(256) k_render(G g, RenderCam cam, RenderPlanes out, RenderStatsDev* __restrict__ stats) {
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
        hit = march(g, cam, r, cc, t_hit, samples);
        float o_n[3] = {0.0f, 0.0f, 0.0f}; float o_alb = 0.0f, o_sh = 0.0f, o_int = 0.0f, o_res = 0.0f;
        if (hit) {
            double w[8]; tri_weights(cc.f, w);
            double gr[3]; cell_gradient(cc, gr);
            const double nx = gr[0], ny = gr[1], nz = gr[2];
            const double nl = sqrt((nx * nx + ny * ny) + nz * nz);
            double n[3] = {0.0, 0.0, 0.0};
            if (nl > 0.0) { n[0] = nx / nl; n[1] = ny / nl; n[2] = nz / nl; }
            double alb = 0.0;
            double shade = 0.0;
            if constexpr (ATTRIBUTES) {
            if (out.albedo || out.need_sh) { double a[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) a[i] = g.alb[cc.c[i]];
                alb = tri_sum(w, a); }
            if (out.need_sh && nl > 0.0) {
                const double H[9] = {1.0, n[1], n[2], n[0], n[0] * n[1], n[1] * n[2], -n[0] * n[0] - n[1] * n[1] + 2.0 * n[2] * n[2], n[0] * n[2], n[0] * n[0] - n[1] * n[1]};
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    double s[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) s[i] = (double)g.sh[(size_t)j * g.N + cc.c[i]];
                    shade = shade + tri_sum(w, s) * H[j];
                }
            }
            }
            o_n[0] = (float)n[0]; o_n[1] = (float)n[1]; o_n[2] = (float)n[2];
            o_alb = (float)alb; o_sh = (float)shade; o_int = (float)(alb * shade);
            if (ATTRIBUTES && out.residual) { o_res = o_int - out.lum[(size_t)v * cam.k.w + u]; rsq = (double)o_res * (double)o_res; }
        }
        const size_t px = (size_t)v * cam.k.w + u;
        if (out.depth) out.depth[px] = hit ? (float)t_hit : 0.0f;
        if (out.normal) { out.normal[3 * px] = o_n[0]; out.normal[3 * px + 1] = o_n[1]; out.normal[3 * px + 2] = o_n[2]; }
        if (out.albedo) out.albedo[px] = o_alb;
        if (out.shading) out.shading[px] = o_sh;
        if (out.intensity) out.intensity[px] = o_int;
        if (out.residual) out.residual[px] = o_res;
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

}  // namespace i3d
