// Registration of depth frames on the stored field (i3d_track_frame_sdf and its batch, rgbd and fusion forms; the definition is DESIGN.md section 19).
//   k_track_sdf_mean       the pivot: per workgroup the sum and the number of the back-projected points of the usable samples that count, one slab row
//   k_track_sdf<G, HUBER, PHOTO>  one lane per sample of the depth image (P samples per lane when the slab would exceed the row cap), 256 lanes per workgroup:
//                          the fp32 depth read from the device copy of the image, the renderer's undistorted ray of the pixel, the point placed by the pose of
//                          the device state, then k_register's cell, residual and Jacobian; with HUBER the 27 entries of the system carry the weight
//                          min(1, k / |r|).  The points are never written to memory.  G = RenderGrid (the context's grid) or FusionRenderGrid (the fusion table
//                          as it stands).  PHOTO: the geometric contribution scaled by wg2, then the intensity volume sampled over the
//                          same cell with the same weights, r_p = I_m - luminance, the Jacobian row with grad c in place of grad f, scaled by wp2
//                          Both kernels have one form: blockIdx.y is the frame, whose image, luminance, state, pivot and slab come from
//                          the device arrays of a TrackSdfBatch.  A single frame is a batch of one, so a frame in a batch gets the bits of its own call
//   k_voxel_intensity      the volume of i3d_track_frame_sdf_rgbd: one lane per stored voxel, albedo x SH shading at the central-difference normal, one fp64
//                          store; a quiet NaN where a neighbour is missing
//   k_fusion_voxel_luminance  the volume of i3d_fusion_track_sdf_rgbd: one lane per table slot, the luminance of the fused colour in fp32,
//                          one fp64 store; a quiet NaN where the slot is empty or has weight 0.  With G = FusionRenderGrid the cell's corners are table slots
//   k_fusion_luminance_lookup  tests only: that volume at given voxel keys
// The rows are totalled and the 6x6 step taken by k_track_solve (track_kernels.hip).  No floating-point atomics: every sum has an order that depends on the
// number of samples alone.  Compiled with -ffp-contract=off: the numpy statement of the definition (tests/track_sdf_twin.py) evaluates the same fp64 expressions
// in the same order.
#include "track_sdf_kernels.hpp"
#include "point_cell_device.hpp"
#include "slab_device.hpp"
#include <type_traits>

namespace i3d {
namespace {

// the camera-frame point of sample i; false when its depth is not usable (not finite, <= 0, outside the depth range)
__device__ inline bool sample_point(const TrackSdfParams& prm, const float* __restrict__ depth, long long i, double (&p)[3]) {
    const int us = (int)(i % prm.ws), vs = (int)(i / prm.ws);
    const int u = us * prm.stride, v = vs * prm.stride;             // u <= (ws - 1) stride < w, v likewise: inside the image
    const float z = depth[(size_t)v * prm.cam.w + u];
    if (!isfinite(z) || !(z > 0.0f) || (prm.min_depth > 0.0f && z < prm.min_depth) || (prm.max_depth > 0.0f && z > prm.max_depth)) return false;
    double x, y; undistort(prm.cam, u, v, x, y);
    const double zd = (double)z;
    p[0] = x * zd; p[1] = y * zd; p[2] = zd;
    return true;
}

// the pivot sums of a workgroup's samples
__device__ inline void mean_sums(const TrackSdfParams& prm, const double (&R)[9], const double (&t)[3], double vs, const float* __restrict__ depth,
                                 double (&s)[TRACK_COLS]) {
#pragma unroll
    for (int k = 0; k < TRACK_COLS; ++k) s[k] = 0.0;
    const long long base = (long long)blockIdx.x * REGISTER_BLOCK * prm.per_lane + threadIdx.x;
    for (int j = 0; j < prm.per_lane; ++j) {
        const long long i = base + (long long)j * REGISTER_BLOCK;
        if (i < prm.n) {                             // tail lanes fall through to the shuffles with zeros
            double p[3];
            bool ok = sample_point(prm, depth, i, p);
            if (ok) {
                s[TRACK_SDF_MEAN_COL_USABLE] = s[TRACK_SDF_MEAN_COL_USABLE] + 1.0;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double x = ((R[3 * a] * p[0] + R[3 * a + 1] * p[1]) + R[3 * a + 2] * p[2]) + t[a];
                    ok = ok && isfinite(x) && fabs(x / vs) < QUERY_MAX_COORD;
                }
            }
            if (ok) { s[0] = s[0] + p[0]; s[1] = s[1] + p[1]; s[2] = s[2] + p[2]; s[3] = s[3] + 1.0; }
        }
    }
}

// blockIdx.y is the frame, blockIdx.x its slab row: the frame's image, pose and slab come from device arrays by a wave-uniform index (scalar loads)
__global__ void __launch_bounds__(REGISTER_BLOCK) k_track_sdf_mean(TrackSdfParams prm, TrackSdfBatch b, double vs) {
    __shared__ double part[REGISTER_BLOCK / 64][TRACK_COLS];
    const int f = blockIdx.y;
    const TrackState* __restrict__ st = b.state + f;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = st->R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = st->t[i];
    double s[TRACK_COLS];
    mean_sums(prm, R, t, vs, b.depth[f], s);
    slab_row(s, part, b.slab + (size_t)f * gridDim.x * TRACK_COLS);
}

// the 29 + 2 sums of a workgroup's samples at the pose R, t about the pivot c.  PHOTO (section 21): the system is wg2 x the geometric one + wp2 x the photometric
// one, columns 30 / 31 are the photometric r^2 and sample count and the usable count is not kept
template <class G, bool HUBER, bool PHOTO>
__device__ inline void track_sdf_sums(const G& g, const TrackSdfParams& prm, const double (&c)[3], const float* __restrict__ depth, const double (&R)[9],
                                      const double (&t)[3], double (&s)[TRACK_COLS], const TrackSdfPhoto& ph, const float* __restrict__ lum) {
    const double vs = g.vs;
#pragma unroll
    for (int k = 0; k < TRACK_COLS; ++k) s[k] = 0.0;
    const long long base = (long long)blockIdx.x * REGISTER_BLOCK * prm.per_lane + threadIdx.x;
    for (int j = 0; j < prm.per_lane; ++j) {
        const long long i = base + (long long)j * REGISTER_BLOCK;
        if (i >= prm.n) break;                       // tail lanes fall through to the shuffles with zeros
        double p[3];
        if (!sample_point(prm, depth, i, p)) continue;
        if constexpr (!PHOTO) s[TRACK_SDF_COL_USABLE] = s[TRACK_SDF_COL_USABLE] + 1.0;
        double xp[3], x[3];                          // only the point stays live across the cell lookup: the ray is spent
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            xp[a] = ((R[3 * a] * p[0] + R[3 * a + 1] * p[1]) + R[3 * a + 2] * p[2]) + t[a];
            x[a] = xp[a] + c[a];
        }
        CellCache cc; cell_cache_reset(cc);
        if (!cell_of_point(g, cc, x)) continue;
        s[29] = s[29] + 1.0;
        const double r = field(cc);
        if (!(fabs(r) <= prm.max_distance)) continue;
        double gr[3]; cell_gradient(cc, gr);
        const double d0 = gr[0] / vs, d1 = gr[1] / vs, d2 = gr[2] / vs;
        const double J[6] = {xp[1] * d2 - xp[2] * d1, xp[2] * d0 - xp[0] * d2, xp[0] * d1 - xp[1] * d0, d0, d1, d2};
        if constexpr (PHOTO) {
            const double wg2 = ph.wg2, ar = fabs(r), om = !HUBER || ar <= prm.huber_delta ? 1.0 : prm.huber_delta / ar;      // 1 (om x) is om x: one text
            add_normal_row(s, J, r, 27, [wg2, om](double x) { return wg2 * (om * x); });
            if (!ph.vol) continue;                   // photo weight 0: no photometric block
            // the intensity volume over the cell the cache holds: from here on cc.v are the eight c values and the geometric row is dead
            bool fin = true;
#pragma unroll
            for (int q = 0; q < 8; ++q) { cc.v[q] = ph.vol[cc.c[q]]; fin = fin && isfinite(cc.v[q]); }
            if (!fin) continue;
            const int us = (int)(i % prm.ws), vs_ = (int)(i / prm.ws);
            const float lf = lum[(size_t)(vs_ * prm.stride) * prm.cam.w + us * prm.stride];
            if (!isfinite(lf)) continue;
            const double rp = field(cc) - (double)lf;
            if (ph.max_residual > 0.0 && !(fabs(rp) <= ph.max_residual)) continue;
            double ge[3]; cell_gradient(cc, ge);
            const double e0 = ge[0] / vs, e1 = ge[1] / vs, e2 = ge[2] / vs;
            const double Jp[6] = {xp[1] * e2 - xp[2] * e1, xp[2] * e0 - xp[0] * e2, xp[0] * e1 - xp[1] * e0, e0, e1, e2};
            const double wp2 = ph.wp2;
            add_normal_row(s, Jp, rp, TRACK_COL_PHOTO_SQ, [wp2](double x) { return wp2 * x; });
        } else if constexpr (HUBER) {
            const double ar = fabs(r), om = ar <= prm.huber_delta ? 1.0 : prm.huber_delta / ar;
            add_normal_row(s, J, r, 27, [om](double x) { return om * x; });
        } else {
            add_normal_row(s, J, r, 27, [](double x) { return x; });
        }
    }
}

// blockIdx.y is the frame, blockIdx.x its slab row: the frame's image, luminance, state, pivot and slab come from device arrays by a wave-uniform index (scalar
// loads).  The workgroups of a frame that is done return at once.  ph is read with PHOTO only
template <class G, bool HUBER, bool PHOTO>
__global__ void __launch_bounds__(REGISTER_BLOCK) k_track_sdf(G g, TrackSdfParams prm, TrackSdfPhoto ph, TrackSdfBatch b, int check_done) {
    __shared__ double part[REGISTER_BLOCK / 64][TRACK_COLS];
    const int f = blockIdx.y;
    const TrackState* __restrict__ st = b.state + f;
    if (check_done && st->done) return;
    // Register allocation, nothing else: without it the depth-only pass over the table reloads the table's base pointers from the kernel arguments inside every
    // hash probe, now that the pivot and the image pointer are values from memory, and a live pass of i3d_fusion_track_sdf takes 2.5 % longer
    if constexpr (std::is_same_v<G, FusionRenderGrid> && !PHOTO) asm("" : "+s"(g.t.keys));
    double R[9], t[3], c[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = st->R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { t[i] = st->t[i]; c[i] = b.pivot[3 * f + i]; }
    double s[TRACK_COLS];
    track_sdf_sums<G, HUBER, PHOTO>(g, prm, c, b.depth[f], R, t, s, ph, PHOTO ? b.lum[f] : nullptr);
    slab_row(s, part, b.slab + (size_t)f * gridDim.x * TRACK_COLS);
}

// one lane per stored voxel (section 21.1 item 1): the normal from the central differences of the field over the six axis neighbours, the renderer's nine basis
// values, the shading summed in fp64 in the order j = 0 .. 8, times the albedo.  Streaming work: every read of the voxel's own planes is coalesced
__global__ void __launch_bounds__(256) k_voxel_intensity(RenderGrid g, double* __restrict__ out) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= g.N) return;
    const size_t N = (size_t)g.N;
    double c = __builtin_nan("");
    if (g.weight[s] != 0.0f) {
        int nb[6];
        bool ok = true;
#pragma unroll
        for (int i = 0; i < 6; ++i) { nb[i] = g.nbr[(size_t)(NB_PX + i) * N + s]; ok = ok && nb[i] >= 0; }
        if (ok) {
#pragma unroll
            for (int i = 0; i < 6; ++i) ok = ok && g.weight[nb[i]] != 0.0f;
        }
        if (ok) {
            const double gx = g.sdf[nb[0]] - g.sdf[nb[1]], gy = g.sdf[nb[2]] - g.sdf[nb[3]], gz = g.sdf[nb[4]] - g.sdf[nb[5]];
            const double nl = sqrt((gx * gx + gy * gy) + gz * gz);
            if (nl > 0.0) {
                const double n[3] = {gx / nl, gy / nl, gz / nl};
                const double H[9] = {1.0, n[1], n[2], n[0], n[0] * n[1], n[1] * n[2], -n[0] * n[0] - n[1] * n[1] + 2.0 * n[2] * n[2], n[0] * n[2], n[0] * n[0] - n[1] * n[1]};
                double shade = 0.0;
#pragma unroll
                for (int j = 0; j < 9; ++j) shade = shade + (double)g.sh[(size_t)j * N + s] * H[j];
                c = g.alb[s] * shade;
            }
        }
    }
    out[s] = c;
}

// one lane per table slot (section 22.1 item 1): k_lum_from_bgr's fp32 operations in its order on the fused R, G, B.  Streaming work: 16 B in, 8 B out per slot
__global__ void __launch_bounds__(256) k_fusion_voxel_luminance(FusionTable t, double* __restrict__ out) {
    const unsigned long long s = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (s > t.mask) return;
    double c = __builtin_nan("");
    if (t.keys[s] != FUSION_EMPTY && t.weight[s] != 0.0f) {
        const uchar4 col = t.color[s];
        const float k = (float)(1.0 / 255.0);
        const float r = (float)col.x * k, g = (float)col.y * k, b = (float)col.z * k;
        c = (double)((b * 0.114f + g * 0.587f) + r * 0.299f);
    }
    out[s] = c;
}

// one lane per requested key: the value of its slot, a quiet NaN when the key is not stored (or cannot be packed)
__global__ void __launch_bounds__(256) k_fusion_luminance_lookup(FusionTable t, const double* __restrict__ vol, long long n, const int* __restrict__ keys,
                                                                 double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    constexpr int K = FUSION_COORD_OFFSET;
    const int x = keys[3 * i], y = keys[3 * i + 1], z = keys[3 * i + 2];
    double c = __builtin_nan("");
    if (x >= -K && y >= -K && z >= -K && x < K && y < K && z < K) {
        const long long s = fusion_hash::find_slot(t, fusion_hash::pack_key(x, y, z));
        if (s >= 0) c = vol[s];
    }
    out[i] = c;
}

template <class G, bool PHOTO>
void launch_sums(hipStream_t st, const G& g, const TrackSdfParams& p, const TrackSdfPhoto& ph, const TrackSdfBatch& b, int check_done) {
    const int rows = register_rows(p.n, p.per_lane);
    if (rows <= 0 || b.frames <= 0) return;
    const dim3 grid(rows, b.frames);
    if (p.huber_delta > 0.0) k_track_sdf<G, true, PHOTO><<<grid, REGISTER_BLOCK, 0, st>>>(g, p, ph, b, check_done);
    else k_track_sdf<G, false, PHOTO><<<grid, REGISTER_BLOCK, 0, st>>>(g, p, ph, b, check_done);
}

template <class G>
void launch(hipStream_t st, const G& g, const TrackSdfParams& p, const TrackSdfPhoto* photo, const TrackSdfBatch& b, int check_done) {
    if (photo) launch_sums<G, true>(st, g, p, *photo, b, check_done);
    else launch_sums<G, false>(st, g, p, TrackSdfPhoto{nullptr, 0.0, 0.0, 0.0}, b, check_done);
}

}  // namespace

void launch_track_sdf_mean(hipStream_t st, const TrackSdfParams& p, const TrackSdfBatch& b, double vs) {
    const int rows = register_rows(p.n, p.per_lane);
    if (rows > 0 && b.frames > 0) k_track_sdf_mean<<<dim3(rows, b.frames), REGISTER_BLOCK, 0, st>>>(p, b, vs);
}
void launch_track_sdf(hipStream_t st, const RenderGrid& g, const TrackSdfParams& p, const TrackSdfPhoto* photo, const TrackSdfBatch& b, int check_done) {
    launch(st, g, p, photo, b, check_done);
}
void launch_track_sdf(hipStream_t st, const FusionRenderGrid& g, const TrackSdfParams& p, const TrackSdfPhoto* photo, const TrackSdfBatch& b, int check_done) {
    launch(st, g, p, photo, b, check_done);
}
void launch_voxel_intensity(hipStream_t st, const RenderGrid& g, double* out) {
    if (g.N > 0) k_voxel_intensity<<<(g.N + 255) / 256, 256, 0, st>>>(g, out);
}
void launch_fusion_voxel_luminance(hipStream_t st, const FusionTable& t, double* out) {
    k_fusion_voxel_luminance<<<(unsigned)((t.mask + 256) / 256), 256, 0, st>>>(t, out);
}
void launch_fusion_luminance_lookup(hipStream_t st, const FusionTable& t, const double* vol, long long n, const int* keys, double* out) {
    if (n > 0) k_fusion_luminance_lookup<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(t, vol, n, keys, out);
}

}  // namespace i3d
